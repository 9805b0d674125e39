/*
 * sfmhip.h — C-ABI of libsfmhip.so, the MI355X (gfx950) backend for the dense
 * compute path of daovietanh190499/3D_Reconstruction (SfM matching, DLT
 * triangulation, reprojection residual / FD Jacobian, voxel-grid work).
 *
 * Conventions (all entry points):
 *   - Every pointer argument that names device data is a HIP device pointer owned
 *     by the caller (normally a torch-ROCm tensor's data_ptr()); the library never
 *     allocates, frees or retains caller memory.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Calls are
 *     asynchronous on that stream; the Python wrappers synchronise before handing
 *     numpy arrays back, which keeps the cv2 / scipy call semantics.
 *   - Return value: 0 on success, a negative SFMHIP_E_* code on failure; the
 *     message for the calling thread is in sfmhip_last_error().
 *   - Row-major, densely packed arrays unless a stride is given.
 *   - An empty call (zero observations / pairs / rays / points / frames) is a no-op
 *     returning 0, and the arrays of that count may then be null (an empty torch
 *     tensor's data_ptr() is 0); shapes and counts are still validated first.
 *
 * Each entry point cites the reference interface it replaces (file:line in
 * /root/reference).  See INTEGRATION.md for the ctypes binding.
 */
#ifndef SFMHIP_H
#define SFMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFMHIP_OK            0
#define SFMHIP_E_ARG        -1   /* bad argument (shape, null pointer, range) */
#define SFMHIP_E_HIP        -2   /* HIP runtime error (launch / memory)        */
#define SFMHIP_E_UNSUPPORTED -3  /* e.g. descriptor dim not in {64,128,256}    */
#define SFMHIP_E_OVERFLOW   -4   /* a bounded loop hit its cap                 */
#define SFMHIP_E_COMM       -5   /* RCCL reported an error                      */

/* element types of sfmhip_allgather */
#define SFMHIP_DT_INT8    0
#define SFMHIP_DT_UINT8   1
#define SFMHIP_DT_INT16   2
#define SFMHIP_DT_INT32   3
#define SFMHIP_DT_INT64   4
#define SFMHIP_DT_FLOAT32 5
#define SFMHIP_DT_FLOAT64 6

/* ---- library ---------------------------------------------------------- */
int         sfmhip_version(void);            /* (major<<16)|(minor<<8)|patch */
const char* sfmhip_last_error(void);         /* thread-local message          */
int         sfmhip_device_arch(char* buf, int len); /* "gfx950" of device 0   */

/* Stream-ordered scratch comes from a library-owned memory pool per device
 * (never the device's default pool); up to 1 GiB of freed scratch stays
 * mapped between calls, and buffers up to 256 MB (1 GiB in all) are cached
 * per (device, stream) so the next call on that stream re-uses them without
 * waiting.  Releases the idle cached buffers of the current device (after a
 * device synchronisation), then trims its pool to `keep` bytes.             */
int         sfmhip_scratch_trim(uint64_t keep);
/* Releases the idle scratch cached for `stream`.  Call it before destroying a
 * stream that was passed to the library (a destroyed stream's buffers are
 * otherwise freed at the next eviction or trim, after a device sync).      */
int         sfmhip_scratch_release_stream(void* stream);
/* Runtime knobs (INTEGRATION.md "Runtime knobs") are read from the environment
 * once, at the first call; this re-reads them (tests switching a knob).      */
int         sfmhip_knobs_reload(void);

/* ---- M1: brute-force L2 matching + ratio test --------------------------
 * Replaces the matcher call site matching.py:20,122-128 (LightGlue forward,
 * output contract lightglue/lightglue.py:442-450).  The BF-L2 + Lowe-ratio
 * semantics are build-defined and pinned by oracle/match.py.
 *
 * Descriptors live in HBM as int8 [n_img][m_pad][d], rows >= n_kpts[img] zero.
 *   mode 0 (SIFT-like, integer values 0..255 stored as f32):  q = x - 128
 *   mode 1 (float, e.g. L2-normalised SuperPoint/DISK):       q = clamp(rint(127*x), -127, 127)
 * Squared L2 on q is exact in int32 (|q|<=128, d<=256).                       */
int sfmhip_desc_quantize(const float* in, int n_img, int m_pad, int d,
                         const int32_t* n_kpts /* device [n_img] */, int mode,
                         int8_t* out /* [n_img][m_pad][d] */, void* stream);

/* norms[img][r] = sum_k q^2 (int32); keys[img][r] = packed column key used by
 * the matcher's fused epilogue (see DESIGN.md "packed key").                  */
int sfmhip_desc_prepare(const int8_t* desc, int n_img, int m_pad, int d,
                        const int32_t* n_kpts, int32_t* norms, int32_t* keys,
                        void* stream);

/* Same as sfmhip_desc_prepare, plus a shifted operand copy for the matcher:
 * desc_shifted = q + shift on valid rows (0 on padding rows), norms and keys
 * adjusted so that sfmhip_match_pairs on (desc_shifted, norms, keys) returns
 * exactly the matches and distances of the unshifted q.  shift in [0, 127];
 * caller guarantees q + shift <= 127 for every valid element (shift 64:
 * q <= 63).
 * Speed only (lower MFMA switching power).                      */
int sfmhip_desc_prepare_shifted(const int8_t* desc, int n_img, int m_pad, int d,
                                const int32_t* n_kpts, int shift, int8_t* desc_shifted,
                                int32_t* norms, int32_t* keys, void* stream);

/* For every pair p=(a,b) and every row i < n_kpts[a] of image a: best column j1
 * (lowest index on ties) and second-best distance d2 over j != j1 in image b.
 * matches0[p][i] = j1 if ratio_den^2 * d1 < ratio_num^2 * d2 (exact, int64)
 * and n_kpts[b] >= 2, else -1; rows i >= n_kpts[a] get -1.
 * dist1/dist2 (nullable) receive d1/d2 (squared, quantised units).
 * m_pad must be a multiple of 128; d in {64,128,256}.                        */
int sfmhip_match_pairs(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                       const int32_t* n_kpts, int n_img, int m_pad, int d,
                       const int32_t* pairs /* device [P][2] */, int P,
                       int ratio_num, int ratio_den,
                       int32_t* matches0 /* [P][m_pad] */,
                       int32_t* dist1, int32_t* dist2, void* stream);

/* The same graph written as int16 (the all-gathered match graph of SURVEY.md §8e,
 * replacing the matching.py:122-128 per-pair LightGlue call over every pair):
 * matches0 entries are identical values; m_pad <= 32767; no distance outputs.  */
int sfmhip_match_pairs_i16(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                           const int32_t* n_kpts, int n_img, int m_pad, int d,
                           const int32_t* pairs, int P, int ratio_num, int ratio_den,
                           int16_t* matches0 /* [P][m_pad] */, void* stream);

/* LightGlue-style mutual filter (lightglue/lightglue.py:235-254 semantics):
 * given forward matches0 (a->b) and backward matches1 (b->a), both [P][m_pad],
 * clear every match that is not mutual, in place.                           */
int sfmhip_mutual_filter(int32_t* matches0, int32_t* matches1, int P, int m_pad,
                         void* stream);

/* Exact float mode (matching.py:111-122 feeds FLOAT DISK / SuperPoint
 * descriptors to the matcher).  Semantics (oracle/match.py bf_match_exact):
 * d(i,j) = sum_k (f64(x_ai,k) - f64(x_bj,k))^2 in k order, one IEEE f64 op
 * per step; j1 = lowest index attaining the minimum, d2 = min over j != j1;
 * accept iff ratio_den^2 * d1 < ratio_num^2 * d2 exactly.
 * sfmhip_desc_residual: per-row bound resid_row [n_img][m_pad] >= |x - v(q)|
 * (v(q) = q/127 for mode 1, q + 128 for mode 0; the int8 q of
 * sfmhip_desc_quantize) and resid_img [n_img] = the image's maximum.          */
int sfmhip_desc_residual(const float* desc_f /* [n_img][m_pad][d] */, const int8_t* desc_q, int n_img, int m_pad,
                         int d, const int32_t* n_kpts, int mode, double* resid_row, double* resid_img,
                         void* stream);

/* The int8 MFMA pass (desc/norms/keys as for sfmhip_match_pairs, shifted or
 * not) certifies every row whose outcome the residual bound decides; the rest
 * are settled against desc_f (f32) by an exact pass over the int8 candidates
 * that can still reach the top two.  matches0 is bit-identical to the exact
 * definition above; dist1/dist2 (nullable) are the int8 pass's quantised
 * distances; n_resolved (nullable, device uint32) = rows the exact pass
 * settled.  desc_q = the unshifted int8 descriptors.                         */
int sfmhip_match_pairs_exact(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                             const int8_t* desc_q, const float* desc_f, const double* resid_row,
                             const double* resid_img, int mode, const int32_t* n_kpts, int n_img, int m_pad, int d,
                             const int32_t* pairs, int P, int ratio_num, int ratio_den,
                             int32_t* matches0, int32_t* dist1, int32_t* dist2, uint32_t* n_resolved,
                             void* stream);

/* sfmhip_match_pairs_exact writing the int16 graph directly (the bench's and
 * dist.match_all_pairs_sharded's graph dtype while m_pad <= 32767; matching.py:122-128
 * over every pair): the same matches0 values, no distance outputs.  Undecided rows
 * carry ceil(8 sqrt(D2)) in their transient mark instead of D2 (a wider candidate
 * radius for the exact pass, never a different result).                      */
int sfmhip_match_pairs_exact_i16(const int8_t* desc, const int32_t* norms, const int32_t* keys,
                                 const int8_t* desc_q, const float* desc_f, const double* resid_row,
                                 const double* resid_img, int mode, const int32_t* n_kpts, int n_img, int m_pad,
                                 int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                 int16_t* matches0, uint32_t* n_resolved, void* stream);

/* The exact float mode with an FP6 (e2m3) certified filter for mode 1, d in
 * {128, 256} (DESIGN.md K1''): the same graph, the filter's dot products on the
 * scaled FP6 MFMA.  sfmhip_desc_quantize_fp6: g [n_img][m_pad][d] int8 = the point
 * of the grid G = {0..15 step 1, 16..30 step 2, 32..60 step 4} (both signs)
 * nearest to the f32 product 127 * x, clipped at +-60; ties go to the even 6-bit
 * code; padded rows 0.  code [n_img][m_pad][d] bytes: per 32 elements one 32-byte
 * chunk, the 6-bit codes (sign << 5 | exponent << 3 | mantissa, bias 1, value
 * g / 8; g = 0 is code 0) at bits 6 e .. 6 e + 5 of its first 24 bytes, little
 * endian, the last 8 bytes zero.  d % 32 == 0.
 * sfmhip_desc_pack_fp6: the operand rows the match kernel reads, built once per
 * bank from `code`.  dense [n_img][m_pad][3 d / 4] bytes, no padding.  Slot s
 * (s = 0 .. d / 32 - 1) of a row is the 24 code bytes of the row's chunk s (codes
 * 32 s .. 32 s + 31), split in two naturally aligned pieces:
 *   low  piece, 16 bytes = chunk bytes 0 .. 15,  at row byte 16 s;
 *   high piece,  8 bytes = chunk bytes 16 .. 23, at row byte d / 2 + 8 s.
 * So a row is its d / 32 low pieces (d / 2 bytes) followed by its d / 32 high
 * pieces (d / 4 bytes): 192 bytes at d = 256, 96 at d = 128.  d % 64 == 0.
 * The match entries take `dense` as their first pointer, norms / keys from
 * sfmhip_desc_prepare on g and the residual bounds from sfmhip_desc_residual on
 * (desc_f, g, mode 1); v(g) = g / 127.
 * No distance outputs.  SFMHIP_MATCH_FP6=0 runs the int8 kernel on g instead.   */
int sfmhip_desc_quantize_fp6(const float* in, int n_img, int m_pad, int d, const int32_t* n_kpts,
                             int8_t* g, uint8_t* code, void* stream);
int sfmhip_desc_pack_fp6(const uint8_t* code, int n_img, int m_pad, int d, uint8_t* dense, void* stream);
int sfmhip_match_pairs_exact_fp6(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                 const int32_t* keys, const float* desc_f, const double* resid_row,
                                 const double* resid_img, const int32_t* n_kpts, int n_img, int m_pad,
                                 int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                 int32_t* matches0, uint32_t* n_resolved, void* stream);
int sfmhip_match_pairs_exact_fp6_i16(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                     const int32_t* keys, const float* desc_f, const double* resid_row,
                                     const double* resid_img, const int32_t* n_kpts, int n_img, int m_pad,
                                     int d, const int32_t* pairs, int P, int ratio_num, int ratio_den,
                                     int16_t* matches0, uint32_t* n_resolved, void* stream);

/* The two entries above derive, on every call, the key values of the whole bank
 * from `keys`: h = keys >> 8 (int32) and hf = h / 64 (f32, exact: |h| <= 2^23),
 * both [n_img][m_pad], the chain starts of the filter.  They depend on the bank
 * alone.  sfmhip_match_key_values builds them once from the keys of
 * sfmhip_desc_prepare on g; the _kv entries take them in place of `keys` and
 * are otherwise the entries above: the same graph and n_resolved.              */
int sfmhip_match_key_values(const int32_t* keys, int n_img, int m_pad, int32_t* h, float* hf, void* stream);
int sfmhip_match_pairs_exact_fp6_kv(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                    const int32_t* h, const float* hf, const float* desc_f,
                                    const double* resid_row, const double* resid_img, const int32_t* n_kpts,
                                    int n_img, int m_pad, int d, const int32_t* pairs, int P, int ratio_num,
                                    int ratio_den, int32_t* matches0, uint32_t* n_resolved, void* stream);
int sfmhip_match_pairs_exact_fp6_kv_i16(const uint8_t* dense, const int8_t* g, const int32_t* norms,
                                        const int32_t* h, const float* hf, const float* desc_f,
                                        const double* resid_row, const double* resid_img, const int32_t* n_kpts,
                                        int n_img, int m_pad, int d, const int32_t* pairs, int P, int ratio_num,
                                        int ratio_den, int16_t* matches0, uint32_t* n_resolved, void* stream);

/* ---- M2: scipy.cluster.vq.vq (matching.py:27, bow.py:23) ---------------
 * codes[i] = argmin_c sum_k (obs[i,k]-code[c,k])^2 (lowest index on ties),
 * dist[i] = sqrt(min).  f64 throughout.                                      */
int sfmhip_vq(const double* obs, int64_t n_obs, const double* code_book, int n_codes,
              int d, int32_t* codes, double* dist, void* stream);

/* ---- BoW retrieval ---------------------------------
 * Per-image visual-word histograms (matching.py:30-35): codes of all images
 * concatenated, image i owns codes[offsets[i] : offsets[i+1]];
 * hist [n_img][k] int32.                                                      */
int sfmhip_word_histogram(const int32_t* codes, const int64_t* offsets, int n_img, int k,
                          int32_t* hist, void* stream);

/* scipy.cluster.vq.kmeans centroid update (bow.py:23 -> _vq.update_cluster_means):
 * per cluster, the f64 sum of its observations in index order, / count.
 * book [k][d] rows of empty clusters are left untouched; counts [k].
 * n = 0 zeroes counts and leaves book as it is; obs and codes may then be null. */
int sfmhip_kmeans_update(const double* obs, int64_t n, int d, const int32_t* codes, int k,
                         double* book, int32_t* counts, void* stream);

/* ---- match-graph consumer, HOST memory ------------
 * Track bookkeeping of matching.py:146-176 for one candidate pair (ref, id):
 * tracks_* are the per-keypoint 3D-point ids of the two images (-1 = none);
 * idx0/idx1 the pair's matches.  interlace = the count of matching.py:146-158;
 * merge = matching.py:161-176 (updates tracks in place, point_ids[n] out,
 * *next_id advanced).  The reference's p1/p2 index quirks are kept.          */
int sfmhip_track_interlace(const int32_t* tracks_ref, int64_t n_ref, const int32_t* tracks_id, int64_t n_id,
                           const int64_t* idx0, const int64_t* idx1, int64_t n, int64_t* interlaced);
int sfmhip_track_merge(int32_t* tracks_ref, int64_t n_ref, int32_t* tracks_id, int64_t n_id,
                       const int64_t* idx0, const int64_t* idx1, int64_t n, int64_t* next_id,
                       int64_t* point_ids);

/* ---- S2: cv2.triangulatePoints (sfm.py:27) ------------------------------
 * OpenCV DLT: per point a 6x4 system (rows x*p3-p1, y*p3-p2, x*p2-y*p1 per
 * view), right singular vector of the smallest singular value (one-sided
 * Jacobi, f64).  x0/x1 are cv2 layout (2,n); X4 is (4,n), unit norm, X4[3]>=0.
 * Batched form: P is [n_pairs][2][3][4] and pair_of_obs[n] selects the pair
 * (pair_of_obs == NULL means one pair).                                      */
int sfmhip_triangulate_dlt(const double* P, const int32_t* pair_of_obs,
                           const double* x0, const double* x1, int64_t n,
                           double* X4, void* stream);

/* ---- S2b: robust N-view triangulation of tracks (build-defined) -------------
 * S2 gives a track the point of the one pair it was first seen in.  This call estimates
 * every track from all of its observations, some of which may be wrong matches, and
 * reports the point, a status and the inlier set.  The reference has no counterpart.
 * Restated in numpy by tests/tri_ref.py.  f64 arithmetic, one IEEE round-to-nearest
 * step per operation in the order written, no FMA, correctly rounded / and sqrt; no
 * floating-point atomics; every sum runs in the order of the sorted list, so two runs
 * give the same bytes and nothing depends on the launch geometry.  All pointers are
 * device memory unless marked host.
 *
 * Inputs.  poses [C][3][4] f64 world -> camera; cam [C][4] f64 = fx, fy, cx, cy; the
 *   observations sorted by (track, camera) in the layout of sfmhip_ba_global*: pt_off
 *   [N+1] i64, obs_cam [M] i32, pts2d [M][2] f64; a repeated (track, camera) pair is legal
 *   and keeps the caller's order.  Track t has the L = pt_off[t+1] - pt_off[t]
 *   observations at positions 0..L-1 of its segment.  A segment that is not inside
 *   [0, M], is reversed or is longer than 2^20 is an empty track; an observation whose
 *   camera is outside [0, C) is not an observation (never an inlier, residual NaN).
 *   The segments must not overlap (pt_off non-decreasing, as the layout implies): every
 *   track keeps its working set in its own range of `inlier`, so two tracks that share
 *   observations read and write nothing out of bounds but leave an undefined result in
 *   both.  track_order [N] i32 or NULL: the order in which the fit kernel's lanes take
 *   the tracks (speed only: descending length keeps a wave's trip counts alike), a
 *   permutation of 0..N-1; an entry outside [0, N) is skipped, a track that is not listed
 *   keeps status 1, and a track listed twice is run by two lanes that share its working
 *   set: undefined for that track like an overlap, in bounds all the same.
 * Parameters.  reproj_px > 0 (thr2 = reproj_px reproj_px); cos_min in (0, 1], the cosine
 *   of the smallest triangulation angle (c2 = cos_min cos_min); 1 <= max_hyp <= 2^20;
 *   refine_iters >= 0.  The device uses no transcendentals.
 * Per camera c_i = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2) is its centre.  For a point X
 *   and an observation (u, v) of camera c with pose rows P0, P1, P2:
 *     xc = ((P00 X0 + P01 X1) + P02 X2) + P03, yc and z likewise;  iz = 1 / z;
 *     du = ((xc iz) fx + cx) - u;  dv = ((yc iz) fy + cy) - v;  e2 = du du + dv dv.
 *   small(a, b, X), the angle at X between the rays to the centres of cameras a and b is
 *   below the minimum:  ra = c_a - X, rb = c_b - X, d = (ra0 rb0 + ra1 rb1) + ra2 rb2,
 *     n = |ra|^2 |rb|^2 (sums in that order);  small iff d > 0 and d d > c2 n.
 * 1. Schedule.  The position pairs (a, b), a < b, in lexicographic order, n_pairs =
 *   L (L - 1) / 2.  n_pairs <= max_hyp: hypothesis h is pair h; else there are max_hyp
 *   hypotheses and hypothesis h is pair floor(h n_pairs / max_hyp) (i64).  A pair whose
 *   observations share a camera, or have one outside [0, C), is skipped.
 * 2. Model (closed form, not S2's DLT): the midpoint of the common perpendicular of the
 *   two viewing rays.  x = (u - cx) / fx, y = (v - cy) / fy; the ray of observation a
 *   leaves c_a along da_i = (R[0][i] x + R[1][i] y) + R[2][i]; w = c_a - c_b; with aa =
 *   da.da, bb = da.db, cc = db.db, dd = da.w, ee = db.w (each (p0 q0 + p1 q1) + p2 q2):
 *     den = aa cc - bb bb;  s = (bb ee - cc dd) / den;  t = (aa ee - bb dd) / den;
 *     X_i = 0.5 ((c_a_i + s da_i) + (c_b_i + t db_i)).
 *   Dropped if a coordinate of X is not finite, if small(a, b, X), or if observation a or
 *   b is not in the set step 3 gives under X.
 * 3. Classification under X.  Observation k is an inlier iff z > 0 and e2 <= thr2 (a NaN
 *   fails; the pixel error is sqrt(e2), so this is error <= reproj_px).  The list is
 *   sorted, so a camera's observations are consecutive: of a camera's inliers only the one
 *   with the smallest e2 stays, the lowest position among equals.  count = the inliers
 *   kept, cost = the sum of their e2 in list order.
 * 4. Winner: the largest count, then the smallest cost, then the lowest h.
 * 5. Fit to a set.  Start: the 4x4 normal matrix of the rows x P2 - P0, y P2 - P1 of the
 *   set's observations (normalised coordinates, summed in list order), its null vector by
 *   the fixed-sweep Jacobi of S2's code, X = y[0..2] / y[3].  Then exactly refine_iters
 *   Gauss-Newton steps on (du, dv): J^T J (3x3) and J^T r summed in list order, the step
 *   by cofactors, X -= step.  X1 is fitted to the winner's set; step 3 under X1 gives the
 *   second set; fewer than two inliers there: status 4.  X2 is fitted to the second set,
 *   which is the reported inlier set.
 * 6. Final tests under X2: every coordinate finite, else 4; z > 0 for every inlier, else
 *   4; some pair of inlier views that is not small(a, b, X2), else 3.
 * Outputs.  X [N][3] f64 (NaN unless OK); status [N] i32: 0 OK, 1 fewer than two distinct
 *   cameras, 2 no hypothesis survived, 3 final angle too small, 4 fit failed; n_inliers
 *   [N] i32 and inlier [M] u8 (0 unless OK); residual [M] f64 = sqrt(e2) under X2 (NaN
 *   where the track is not OK).  n_hyp (host, or NULL): the hypotheses scored.  phase_ms
 *   (host [2], or NULL): when given, the call waits for its kernels and reports the
 *   milliseconds of the scoring and of the select-and-fit kernel (tools only).
 * Kernels: an initialisation (failure values, per-track hypothesis counts, centres), a
 *   one-workgroup integer scan, then the scoring kernel over the flattened hypotheses of
 *   all tracks (one lane per hypothesis, one record of count and cost each) and the
 *   select-and-fit kernel (one lane per track, records scanned in h order).  The call
 *   reads the hypothesis total back once, before the two phases, to size the records
 *   (12 bytes each, from the scratch pool); nothing returns to the host between them.
 * A null pointer or a negative size is SFMHIP_E_ARG, as are max_hyp < 1, refine_iters < 0
 *   and a threshold that is not finite and positive; shapes are checked before the
 *   empty-call no-op: with N = 0, M = 0 or C < 2 every status is 1 and no phase runs.   */
int sfmhip_triangulate_tracks(const double* poses, const double* cam, int C, const int64_t* pt_off, int64_t N,
                              const int32_t* obs_cam, const double* pts2d, int64_t M,
                              const int32_t* track_order, double reproj_px, double cos_min, int max_hyp,
                              int refine_iters, double* X /* [N][3] */, int32_t* status /* [N] */,
                              int32_t* n_inliers /* [N] */, uint8_t* inlier /* [M] */, double* residual /* [M] */,
                              int64_t* n_hyp /* host */, float* phase_ms /* host [2] */, void* stream);

/* ---- S3/S5: reprojection residual + scipy 2-point grouped FD Jacobian ----
 * sfm.py:87-91 (residual via cv2.projectPoints, no distortion) and
 * least_squares(..., jac_sparsity=ba_sparse(...)) sfm.py:37-38.
 * cam: [n_pairs][6] = rvec(3), t(3);  K: [n_pairs][3][3] (fx,fy,cx,cy used);
 * X: [n][3]; pts2d: [n][2]; pair_of_obs: [n] (NULL = one pair).
 * r: [n][2]  residual (pts2d - proj)  (nullable)
 * f0: [n][2] base residual to difference against (NULL = computed here)
 * jvals: [n][2][9] CSR values of J, per row: d/d(rvec0..2,t0..2, X0..2).    */
int sfmhip_reproj_residual(const double* cam, const double* K, const double* X,
                           const double* pts2d, const int32_t* pair_of_obs,
                           int64_t n, double* r, void* stream);
/* HOST arrays (the cv2.projectPoints / calculate_reprojection_error contract
 * sfm.py:87-91, called by scipy's least_squares ~40 times per pair at sfm.py:38):
 * cam[6], K[9], X[n][3], pts2d[n][2] (NULL = zeros, i.e. -projectPoints) and
 * r[n][2] are host memory.  One pinned staging buffer per device (library-owned,
 * grows on demand) that the kernel reads and writes over PCIe (zero-copy), then a synchronisation
 * of `stream`.  Blocking; thread-safe (the staging is locked per device).     */
int sfmhip_reproj_residual_host(const double* cam, const double* K, const double* X,
                                const double* pts2d, int64_t n, double* r, void* stream);
int sfmhip_reproj_fd_jacobian(const double* cam, const double* K, const double* X,
                              const double* pts2d, const int32_t* pair_of_obs,
                              int n_pairs, int64_t n, const double* f0,
                              double* r, double* jvals, void* stream);

/* The BA solve of sfm.py:37-38 (scipy least_squares, method 'trf', tr_solver
 * 'lsmr', jac_sparsity = ba_sparse, x_scale = 'jac', ftol / xtol / gtol) for
 * n_pairs independent problems at once, one workgroup each.  Problem p:
 * x = [cam[p] (rvec 3, t 3), X[off[p]..off[p+1]) (3 each)], residual
 * pts2d - projectPoints(X, rvec, t, K[p]) (calculate_reprojection_error,
 * sfm.py:87-91).  cam (n_pairs, 6) and X (n, 3) are updated in place;
 * pair_off (n_pairs + 1) int64 device offsets (off[0] = 0, observations of a
 * pair contiguous); max_nfev <= 0: scipy's default 100 * len(x).  Outputs per
 * pair: final cost 0.5 |f|^2, nfev, njev, status (scipy's codes 0..4).
 * n_obs = rows of X / pts2d: a pair whose offsets are not
 * 0 <= off[p] <= off[p+1] <= n_obs touches nothing and gets status -1.
 * The Gauss-Newton direction is the exact damped least-squares solution where
 * scipy runs LSMR to 1e-6 (oracle/ba.py). */
int sfmhip_ba_solve(double* cam, const double* K, double* X, const double* pts2d, const int64_t* pair_off,
                    int n_pairs, int64_t n_obs, double ftol, double xtol, double gtol, int max_nfev, double* cost,
                    int32_t* nfev, int32_t* njev, int32_t* status, void* stream);

/* ---- K3''': global bundle adjustment (build-defined, no reference counterpart) ----
 * All C cameras and N points against all M observations: residual
 * project(R_c X_p + t_c) - pts2d, cost 0.5 sum |r|^2, f64 throughout.
 * Levenberg-Marquardt with Marquardt scaling (U + lambda diag U, V + lambda diag V);
 * the reduced camera system S = U* - W V*^-1 W^T is never formed: block-Jacobi
 * preconditioned CG applies it by two segment passes over the stored Jacobians
 * (DESIGN.md K3'''; tests/ba_global_ref.py restates every step).  No floating-point
 * atomics; every sum has a fixed order given by the sorted structure, so two runs
 * give the same bits.
 * cam [C][6] = rvec, t (world -> camera); K [C][3][3] (fx, fy, cx, cy read, fixed);
 * X [N][3].  The observations are held SORTED by (point, camera), repeated pairs in
 * the caller's order: obs_cam, obs_pt [M] int32, pts2d [M][2]; pt_off [N+1] int64
 * (point p owns [pt_off[p], pt_off[p+1])); cam_perm [M] int64 lists, camera by
 * camera and ascending inside a camera, the positions of each camera's
 * observations, cam_off [C+1] int64 its offsets.  cam_fixed [C] uint8 (NULL: none):
 * rows and columns of a fixed camera leave the system, its step is exactly 0.
 * The left perturbation R <- exp(dw) R, t <- t + dt parametrises a camera;
 * Jc [M][2][6] = d r / d (dw, dt), Jp [M][2][3] = d r / d X, analytic.
 * All arrays are device memory except `cost` and `info` (host).
 *
 * sfmhip_ba_global_linearize: r [M][2], Jc, Jp in sorted order, U [C][6][6] =
 * sum Jc^T Jc, g_c [C][6] = sum Jc^T r, V [N][3][3], g_p [N][3], *cost (infinite
 * when an observation has a non-positive depth).  Blocking.
 * sfmhip_ba_global_schur_matvec: out [C][6] = S(lambda) x from those arrays
 * (entries of x at fixed cameras are not read, their rows of out are 0).  lambda >= 0;
 * lambda must be positive when some V is singular (a point with a single observation has a
 * rank-2 V): the damping is what makes V* invertible, at lambda = 0 its inverse is not finite.
 * Sizes: C <= 2^20, M < 2^31, N < 2^27 (all three calls).
 * sfmhip_ba_global: the whole solve; cam and X are updated in place (a fixed camera,
 * a camera without observations and a point without observations come back
 * bit-unchanged).  Per linearisation the damped system is solved by at most max_cg
 * CG iterations to |r_k| <= eta |b|; the step is accepted iff the cost decreases
 * (lambda <- max(lambda / 3, 1e-12), else lambda <- 4 lambda and the same
 * linearisation is solved again), lambda starts at 1e-4.  cost[2] = initial and
 * final cost; info[4] = status, linearisations, accepted steps, CG iterations.
 * status: 1 max |g| <= gtol at an accepted point; 2 relative cost decrease of the
 * last accepted step <= ftol; 0 max_iter linearisations used; 3 lambda > 1e12;
 * -1 an index out of range, offsets not monotone or the orders inconsistent;
 * -2 a non-positive depth at the start (-1, -2: nothing is written).  Blocking:
 * the host reads one control record per trial step, never inside the CG loop.
 * The three calls return SFMHIP_E_ARG for a null pointer or a negative size; the
 * first two also for the structure errors that sfmhip_ba_global reports as -1.  */
int sfmhip_ba_global_linearize(const double* cam, const double* K, const double* X, const int32_t* obs_cam,
                               const int32_t* obs_pt, const double* pts2d, const int64_t* pt_off,
                               const int64_t* cam_perm, const int64_t* cam_off, int C, int N, int64_t M,
                               double* r, double* Jc, double* Jp, double* U, double* g_c, double* V,
                               double* g_p, double* cost, void* stream);
int sfmhip_ba_global_schur_matvec(const double* Jc, const double* Jp, const double* U, const double* V,
                                  const int32_t* obs_cam, const int32_t* obs_pt, const int64_t* pt_off,
                                  const int64_t* cam_perm, const int64_t* cam_off, const uint8_t* cam_fixed,
                                  int C, int N, int64_t M, double lambda, const double* x, double* out,
                                  void* stream);
int sfmhip_ba_global(double* cam, const double* K, double* X, const int32_t* obs_cam, const int32_t* obs_pt,
                     const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm, const int64_t* cam_off,
                     const uint8_t* cam_fixed, int C, int N, int64_t M, double gtol, double ftol, double eta,
                     int max_iter, int max_cg, double* cost, int32_t* info, void* stream);
/* Robust loss (plain IRLS; DESIGN.md K3''' "Robust loss", tests/ba_robust_ref.py).  loss: 0 linear,
 * 1 huber, 2 soft_l1, 3 cauchy; f_scale > 0 in pixels.  The loss acts on the 2-vector of an
 * observation (as Ceres does, not per scalar component as scipy's least_squares does):
 * z = |r|^2 / f_scale^2, cost = 0.5 f_scale^2 sum rho(z) with scipy's rho (huber: z if z <= 1, else
 * 2 sqrt z - 1; soft_l1: 2 (sqrt(1 + z) - 1); cauchy: log1p z), weight w = rho'(z).  The
 * linearisation stores sqrt(w) r, sqrt(w) Jc, sqrt(w) Jp in place of r, Jc, Jp, so blocks, gradient,
 * damping, CG, back-substitution and the step rule are the robust Gauss-Newton ones unchanged; no
 * second-order correction.  loss = 0 runs exactly what the two entries above run (they forward here).
 * sfmhip_ba_global_linearize_robust: as sfmhip_ba_global_linearize, the arrays weighted, *cost the
 * robust cost, weight [M] = w per sorted observation (1 for loss 0).
 * sfmhip_ba_global_robust: as sfmhip_ba_global, cost[2] the robust cost; obs_res2 [M] (device,
 * nullable) receives the final UNWEIGHTED |r|^2 of every sorted observation (not written for
 * status -1 / -2).  An unknown loss code, or f_scale not > 0 or not finite: SFMHIP_E_ARG, checked
 * before anything else.  */
int sfmhip_ba_global_linearize_robust(const double* cam, const double* K, const double* X, const int32_t* obs_cam,
                                      const int32_t* obs_pt, const double* pts2d, const int64_t* pt_off,
                                      const int64_t* cam_perm, const int64_t* cam_off, int C, int N, int64_t M,
                                      double* r, double* Jc, double* Jp, double* U, double* g_c, double* V,
                                      double* g_p, double* cost, void* stream, int loss, double f_scale,
                                      double* weight);
int sfmhip_ba_global_robust(double* cam, const double* K, double* X, const int32_t* obs_cam, const int32_t* obs_pt,
                            const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm,
                            const int64_t* cam_off, const uint8_t* cam_fixed, int C, int N, int64_t M, double gtol,
                            double ftol, double eta, int max_iter, int max_cg, double* cost, int32_t* info,
                            void* stream, int loss, double f_scale, double* obs_res2);

/* ---- K3''' with intrinsics: shared intrinsics and radial distortion as unknowns (ba_calib.hip;
 * DESIGN.md "K3''' with intrinsics", tests/ba_calib_ref.py restates every step).
 * Every camera belongs to one of G intrinsics groups: cam_group [C] int32 in [0, G).  A group holds
 * theta [G][5] = (f, cx, cy, k1, k2) and a fixed aspect asp [G] = fy / fx (zero skew):
 *   (x, y, z) = R X + t, xn = x / z, yn = y / z, r2 = xn^2 + yn^2, d = 1 + k1 r2 + k2 r2^2,
 *   u = f (d xn) + cx, v = (f asp) (d yn) + cy        (OpenCV's radial model with p1 = p2 = k3 = 0).
 * mask [5] uint8 (device, each 0 or 1; the same for every group): 1 = the component of theta is
 * free.  Everything else — the sorted observation layout, cam_fixed, the left perturbation of a
 * camera, the loss codes and f_scale, the step rule, tolerances, cost[2], info[4], the status codes
 * and obs_res2 — is as in sfmhip_ba_global_robust.  The camera-side unknown is x~ = (x_c [6C],
 * x_k [5G]), the intrinsics after the cameras.  No floating-point atomics; a group's sums add the
 * per-camera values in ascending camera index (lane l of 256 takes the group's l-th, (l+256)-th, ...
 * camera in sequence, then the pairwise tree), so two runs give the same bits.
 *
 * sfmhip_ba_calib_linearize: r [M][2], Jc [M][2][6], Jk [M][2][5] = d r / d theta (columns of masked
 * components 0), Jp [M][2][3] in sorted order, weighted by sqrt(w) under a robust loss; U [C][6][6],
 * g_c [C][6], B [C][6][5] = sum Jc^T Jk, H [G][5][5] = sum Jk^T Jk, g_k [G][5] = sum Jk^T r,
 * V [N][3][3], g_p [N][3], *cost, weight [M] (nullable).  Blocking.
 * sfmhip_ba_calib_matvec: out [6C + 5G] = S~(lambda) x~ with
 *   S~ x~ = [U* x_c + B x_k ; sum_c B^T x_c + H* x_k] - A~^T Jp V*^-1 Jp^T A~ x~,  A~ = [Jc | Jk];
 * observations of a fixed camera still act through Jk.  Entries of x at fixed cameras and masked
 * components are not read; their rows of out are exactly 0.
 * sfmhip_ba_calib: the whole solve; cam, theta and X are updated in place.  A fixed camera, a camera
 * or point without observations, a masked component and a group without cameras come back
 * bit-unchanged.  With k1 = k2 = 0, an empty mask and fy == f asp in floating point (square pixels
 * for one) every value equals sfmhip_ba_global_robust's.
 * Sizes: as sfmhip_ba_global, and G <= 2^20; C > 0 needs G > 0.  */
int sfmhip_ba_calib_linearize(const double* cam, const double* theta, const double* asp, const int32_t* cam_group,
                              const uint8_t* mask, const double* X, const int32_t* obs_cam, const int32_t* obs_pt,
                              const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm,
                              const int64_t* cam_off, int C, int N, int G, int64_t M, double* r, double* Jc,
                              double* Jk, double* Jp, double* U, double* g_c, double* B, double* H, double* g_k,
                              double* V, double* g_p, double* cost, void* stream, int loss, double f_scale,
                              double* weight);
int sfmhip_ba_calib_matvec(const double* Jc, const double* Jk, const double* Jp, const double* U, const double* B,
                           const double* H, const double* V, const int32_t* cam_group, const uint8_t* mask,
                           const int32_t* obs_cam, const int32_t* obs_pt, const int64_t* pt_off,
                           const int64_t* cam_perm, const int64_t* cam_off, const uint8_t* cam_fixed, int C, int N,
                           int G, int64_t M, double lambda, const double* x, double* out, void* stream);
int sfmhip_ba_calib(double* cam, double* theta, const double* asp, const int32_t* cam_group, const uint8_t* mask,
                    double* X, const int32_t* obs_cam, const int32_t* obs_pt, const double* pts2d,
                    const int64_t* pt_off, const int64_t* cam_perm, const int64_t* cam_off, const uint8_t* cam_fixed,
                    int C, int N, int G, int64_t M, double gtol, double ftol, double eta, int max_iter, int max_cg,
                    double* cost, int32_t* info, void* stream, int loss, double f_scale, double* obs_res2);
/* Inverse of the radial model above for pixels: src, dst [n][2] (device).  20 fixed-point steps
 * xn <- xd / d(xn) from the distorted normalised point; dst is the pixel under the same fx, fy, cx,
 * cy with zero distortion.  */
int sfmhip_undistort_points(const double* src, int64_t n, double fx, double fy, double cx, double cy, double k1,
                            double k2, double* dst, void* stream);

/* ---- V1: voxel_traversal (voxel_travesal.py:1-73), quirks included -------
 * rays [N][8] f32 = o(3), d(3), near, far.  Pass 1 counts per-ray steps
 * (n_steps[N]; a ray still active after max_steps reports max_steps + 1),
 * pass 2 writes out [N][S][3] f32 (NaN padded) with S = 1 + max(n_steps).   */
int sfmhip_voxel_traversal_count(const float* rays, int64_t N, float bin,
                                 int32_t max_steps, int32_t* n_steps, void* stream);
int sfmhip_voxel_traversal(const float* rays, int64_t N, float bin, int32_t S,
                           float* out, void* stream);
/* One walk instead of two: each ray's visited voxels into rows of width `cap`
 * (buf [N][cap][3]; entries past a row's end are left unwritten) and its step
 * count (n_steps[N]; cap when the ray is still active after cap - 1 steps).
 * When every n_steps < cap, sfmhip_voxel_traversal_rows with S = 1 + max
 * n_steps writes exactly the two-pass form's out [N][S][3] (NaN padded);
 * otherwise the caller falls back to the two-pass form.                    */
int sfmhip_voxel_traversal_capped(const float* rays, int64_t N, float bin, int32_t cap,
                                  float* buf, int32_t* n_steps, void* stream);
int sfmhip_voxel_traversal_rows(const float* buf, int32_t cap, const int32_t* n_steps,
                                int64_t N, int32_t S, float* out, void* stream);

/* ---- V2: trilinear grid sample (sdf.py:284-342, plenoxel.py:31-43) -------
 * grid in the reference layout (1,C,D,H,W) f32.  pts [P][3] world coords.
 * mask_mode 0: sdf.py  (inside iff bmin <= p <= bmax, normalise to [-1,1])
 * mask_mode 1: plenoxel (inside iff |p| < scale=bmax[0], p/scale clipped)
 * out [P][C] (zero outside).  F.grid_sample(align_corners=True, zeros)
 * arithmetic, x->W, y->H, z->D.  bmin/bmax are HOST float[3].  D, H, W >= 1,
 * here and in sfmhip_nerf_forward: an axis of one voxel has index 0.       */
int sfmhip_grid_sample(const float* grid, int C, int D, int H, int W,
                       const float* bmin, const float* bmax, int mask_mode,
                       const float* pts, int64_t P, float* out, void* stream);

/* NerfModel.forward (plenoxel.py:31-43) for C = 28 grids in the reference
 * layout: color [P][3] = eval_spherical_function(channels 1..27, dirs),
 * sigma [P] = ReLU(channel 0), both zero outside the mask (mask_mode as in
 * sfmhip_grid_sample); dirs [P][3].  bmin/bmax are HOST float[3].           */
int sfmhip_nerf_forward(const float* grid, int D, int H, int W, const float* bmin, const float* bmax,
                        int mask_mode, const float* pts, const float* dirs, int64_t P, float* color,
                        float* sigma, void* stream);

/* Voxel-major relayout (C,D,H,W) -> (D,H,W,Cp) with Cp = 32 (zero pad) so a
 * corner's channels are one 128-byte line; used by the fused renderer.       */
int sfmhip_grid_to_voxel_major(const float* grid, int C, int D, int H, int W,
                               float* grid_vm, void* stream);

/* ---- V4: fused sample + SH-2 colour + alpha composite --------------------
 * sdf.py:391-406 / plenoxel.py:71-93 for C=28 grids.  rays_o/rays_d [B][3],
 * z [B][S] (sorted sample depths).  rgb [B][3] = sum T*a*c + 1 - sum T*a.
 * grid_vm from sfmhip_grid_to_voxel_major; bmin/bmax are HOST float[3].     */
int sfmhip_render_rays(const float* grid_vm, int D, int H, int W,
                       const float* bmin, const float* bmax, int mask_mode,
                       const float* rays_o, const float* rays_d, const float* z,
                       int64_t B, int S, float* rgb, void* stream);
/* The same render with the SDF (channel 0) also given as the compact reference
 * plane (D,H,W) f32 (grid channel 0 of the (C,D,H,W) layout): each sample's sdf
 * is read from it and the 28-channel voxel lines are fetched only for samples
 * with alpha != 0 (w = T*alpha = 0 otherwise).  The caller guarantees a finite
 * grid; the result is then bit-identical to sfmhip_render_rays.              */
int sfmhip_render_rays_sdf(const float* grid_vm, const float* sdf_plane, int D, int H, int W,
                           const float* bmin, const float* bmax, int mask_mode,
                           const float* rays_o, const float* rays_d, const float* z,
                           int64_t B, int S, float* rgb, void* stream);

/* ---- V5: TSDF integration (build-defined) --------------
 * T, Wt: (D,H,W) f32 grids updated in place for z-slices [z0, z1), laid out
 * like the sdf.py grid (sdf.py:284-304: x -> W, align_corners).
 * depth [F][Hd][Wd] f32 (<= 0 invalid); poses [F][3][4] world->camera;
 * Kf [F][4] = fx, fy, cx, cy; bmin/bmax are HOST float[3] grid bounds;
 * trunc = truncation distance mu (world units).  The frames of one integration
 * step (the call, in steps of at most 512 frames) are fused order-free: per
 * voxel S = sum rint(tsdf * 2^21) and n updates, then W' = W + n,
 * T' = f32((f64 T * W + S 2^-21) / (W + n))  (oracle/voxel.py tsdf_integrate).
 * F = 0 or z0 = z1: a no-op (with F = 0 the frame arrays may be null).        */
int sfmhip_tsdf_integrate(float* T, float* Wt, int D, int H, int W, int z0, int z1,
                          const float* depth, int F, int Hd, int Wd,
                          const float* poses, const float* Kf,
                          const float* bmin, const float* bmax, float trunc,
                          void* stream);

/* The TSDF pre-pass table on its own, for sharing across ranks (multi-GPU
 * z-slabs: each rank computes the table of a frame range and an all-gather
 * assembles it, instead of every rank reading every depth map): {min, max}
 * of every 16x16 depth block, table [F][ceil(Hd/16)][ceil(Wd/16)][2] f32
 * (min poisoned by NaN, max ignoring NaN); rows [f0, f1) are written.      */
int sfmhip_tsdf_block_table(const float* depth, int F, int Hd, int Wd,
                            int f0, int f1, float* table, void* stream);

/* sfmhip_tsdf_integrate with the caller's full block table (all F frames,
 * whole image, as written by sfmhip_tsdf_block_table): bit-identical
 * result, the call's own block pass skipped.                                 */
int sfmhip_tsdf_integrate_tab(float* T, float* Wt, int D, int H, int W, int z0, int z1,
                              const float* depth, int F, int Hd, int Wd,
                              const float* poses, const float* Kf,
                              const float* bmin, const float* bmax, float trunc,
                              const float* table, void* stream);

/* Diagnostics for the TSDF pre-passes (no reference counterpart): runs only
 * the culling / free-space tests of sfmhip_tsdf_integrate over the same
 * arguments and returns HOST int64 stats[3] = (wave sub-tile, frame) pairs
 * tested, culled (no voxel updates), free space (every voxel updates with
 * tsdf = 1, fused without depth gathers).  Synchronises the stream.         */
int sfmhip_tsdf_cull_stats(int D, int H, int W, int z0, int z1,
                           const float* depth, int F, int Hd, int Wd,
                           const float* poses, const float* Kf,
                           const float* bmin, const float* bmax, float trunc,
                           int64_t* stats, void* stream);

/* Per-layer version for z-slab planning (multi-GPU): the same tests over the
 * whole grid, HOST int64 layer_stats[ceil(D/8)][3] (tested, culled, free) per
 * 8-voxel tile layer in z.  Synchronises the stream.                         */
int sfmhip_tsdf_layer_stats(int D, int H, int W, const float* depth, int F, int Hd, int Wd,
                            const float* poses, const float* Kf, const float* bmin, const float* bmax,
                            float trunc, int64_t* layer_stats, void* stream);

/* ---- V6: triangle mesh of the fused TSDF grid (build-defined) -------------
 * Marching tetrahedra on the Kuhn (Freudenthal) 6-tetrahedron split of every
 * cell: 16 cases per tetrahedron, no ambiguous case, neighbouring cells agree
 * on shared faces, so the mesh is a consistently oriented 2-manifold.  The
 * reference's final artefact is a .ply (sfm.py:54-77, numpy2ply.py); it has no
 * volumetric surface.  Restated in numpy by tests/surface_ref.py.
 *
 * Inputs: T, Wt (D,H,W) f32 as sfmhip_tsdf_integrate leaves them (x -> W,
 * y -> H, z -> D, align_corners; Wt == 0: never observed; T positive in free
 * space); HOST float[3] bounds bmin / bmax; iso; min_weight (<= 0 is
 * SFMHIP_E_ARG); a cell-layer range [z0, z1), 0 <= z0 <= z1 <= D-1.
 *
 * Voxels and cells: voxel (z,y,x) has linear id (z*H + y)*W + x.
 * observed(v): Wt[v] >= min_weight and T[v] finite.  inside(v): T[v] < iso.
 * Cell (z,y,x) exists for z in [z0,z1), y < H-1, x < W-1; its corners are the
 * 8 voxels at offsets in {0,1}^3; it is VALID when all 8 are observed; its
 * linear id is (z*(H-1) + y)*(W-1) + x.
 *
 * Edge slots: each voxel owns 7, slot k with offset (dx,dy,dz):
 *   0 (1,0,0)  1 (0,1,0)  2 (0,0,1)  3 (1,1,0)  4 (1,0,1)  5 (0,1,1)  6 (1,1,1)
 * (every edge of every Kuhn tetrahedron is one of these).  Edge (v,k) is ACTIVE
 * when v+o_k is in the grid, inside(v) != inside(v+o_k), and at least one valid
 * cell of this call's range has both endpoints among its corners (4 candidate
 * cells for axis edges, 2 for face diagonals, 1 for the body diagonal).
 *
 * Vertices: one per active edge, ordered by (voxel linear id, k).  f32, no
 * FMA, op by op: s = (iso - T[v]) / (T[v+o] - T[v]); per axis
 * g = f32(idx) + s*f32(o), p = bmin + g*step, step = (bmax - bmin)/f32(R-1).
 *
 * Normals (optional): for voxel u and axis a the gradient is the central
 * difference (T[u+e_a] - T[u-e_a]) / (2 step_a) when both neighbours are in
 * the grid (the whole grid passed in, not the range) and observed, the
 * one-sided difference over step_a when one is, 0 when neither.  The vertex
 * normal is normalize((1-s) g(v) + s g(v+o)), (0,0,0) when the length is 0 or
 * not finite; it points towards increasing T (free space).
 *
 * Tetrahedra: 6 per cell; tetrahedron t is the lexicographic rank of the axis
 * permutation (a,b,c) of (x,y,z); its corners are c0 (the cell origin),
 * c1 = c0+e_a, c2 = c1+e_b, c3 = c0+(1,1,1).
 *
 * Triangles: only valid cells emit.  With tetrahedron corner indices ascending:
 *   0 or 4 corners inside: nothing;
 *   1 inside (i; outside o1<o2<o3): (i-o1, i-o2, i-o3);
 *   3 inside (i1<i2<i3; outside o): (i1-o, i2-o, i3-o);
 *   2 inside (p<q; outside r<s):    (pr, ps, qs) and (pr, qs, qr);
 * the last two vertices swapped where needed so that (v1-v0)x(v2-v0) points
 * towards the outside corners (a function of (t, case) only: a generated 6x16
 * bit table).  Order: cell linear id, then t, then the order above.  Face
 * indices refer to this call's vertex array.  Zero-area triangles (T == iso at
 * a corner) are kept.
 *
 * Slabs: for any partition of [0, D-1) into ranges, the concatenated per-call
 * triangle soups vertices[faces] (and the normals at those corners) are
 * bit-identical to the whole-grid call's; boundary vertices are duplicated
 * between calls.  A rank needs its slab plus one neighbouring voxel layer
 * (two for identical normals on the boundary layer).
 *
 * Count, then fill (like sfmhip_voxel_traversal_count / _traversal).  The work
 * arrays are the caller's, 16-byte aligned, indexed relative to the range
 * (NV = (z1-z0+1)*H*W voxels of layers z0..z1, NC = (z1-z0)*(H-1)*(W-1) cells):
 *   edge_mask u8 [NV]    bit k = edge (v,k) active
 *   vert_off i32 [NV+1]  first vertex of each voxel; [NV] = total vertices
 *   tri_off  i32 [NC+1]  first triangle of each cell; [NC] = total triangles
 * sfmhip_tsdf_surface_count fills them and returns HOST int64 totals[2] =
 * (vertices, triangles); it synchronises the stream.  A total above INT32_MAX
 * (or NV >= INT32_MAX) is SFMHIP_E_OVERFLOW: split the range.  Deterministic:
 * plain multi-kernel scans, no atomics.
 * sfmhip_tsdf_surface_emit (same grids, range, iso, min_weight and work
 * arrays) writes vertices [V][3] f32, normals [V][3] f32 (nullable) and faces
 * [F][3] i32; vertices / normals / faces may be null when their total is 0.
 * z0 == z1, H == 1 or W == 1: no cells, totals 0, nothing is read or written. */
int sfmhip_tsdf_surface_count(const float* T, const float* Wt, int D, int H, int W, int z0, int z1,
                              float iso, float min_weight, uint8_t* edge_mask, int32_t* vert_off,
                              int32_t* tri_off, int64_t* totals /* HOST [2] */, void* stream);
int sfmhip_tsdf_surface_emit(const float* T, const float* Wt, int D, int H, int W, int z0, int z1,
                             float iso, float min_weight, const float* bmin, const float* bmax,
                             const uint8_t* edge_mask, const int32_t* vert_off, const int32_t* tri_off,
                             float* vertices, float* normals /* nullable */, int32_t* faces, void* stream);

/* ---- V7: TSDF colour fusion (build-defined) --------------------------------
 * Image colour fused beside the distance of V5 and interpolated onto the
 * vertices of V6: the reference's final artefact is a coloured .ply
 * (sfm.py:54-77, numpy2ply.py: xyz + colour).  Restated in numpy by
 * tests/tsdf_colour_ref.py.
 *
 * State: C (D,H,W,4) i32, read and written as u32 with arithmetic modulo 2^32:
 * per voxel {sum_r, sum_g, sum_b, n}, 16 bytes, 16-byte aligned (one 128-bit
 * access per voxel).  A channel sum can pass 2^31 only after 2^23 updates of
 * one voxel (255 * 2^23 < 2^31); n and the sums wrap modulo 2^32 beyond.
 *
 * Input: colour [F][Hd][Wd][4] u8, bytes r, g, b, x (x ignored), pixel-aligned
 * with depth: pixel (v,u) is the dword at the depth gather's own offset.
 *
 * Rule per (voxel, frame): V5 exactly as oracle/voxel.py _tsdf_frames writes
 * it (the same f32 operations in the same order: the frame-skip rule,
 * 2^-60 <= Zc < 2^60, iz = 1/Zc, pixel = floor((fx Xc) iz + (cx + 0.5)),
 * off-image, depth > 0, sdf = depth - Zc, skip sdf < -mu,
 * ts = min(1, sdf (1/mu))).  The voxel takes the frame's colour iff V5 would
 * update it AND ts < 1 (f32 compare): sums += (r, g, b) of that pixel, n += 1.
 * Nothing else: no 512-frame steps, no dependence on T or Wt, and integer sums,
 * so any frame order, any z-slab split and any grouping of the frames into
 * calls give the same bits.  F = 0 or z0 = z1: a no-op.  table: nullable, the
 * caller's block table as for sfmhip_tsdf_integrate_tab (same bits).
 *
 * Vertex colour of an active edge (v,k) of V6 with endpoints v, v+o and V6's
 * own s: per channel col(u) = f32(sum[u]) / f32(n[u]) where n[u] > 0 (u32 ->
 * f32 round-to-nearest, IEEE f32 division); both endpoints coloured:
 * m = a + s (b - a), no FMA; one coloured: m = its col; neither: m = 0 and
 * alpha = 0.  Byte = rint(min(255, max(0, m))), round-half-even; alpha = 255
 * when at least one endpoint is coloured.  rgba [V][4] u8 in vertex order
 * (edge_mask / vert_off as sfmhip_tsdf_surface_count left them for the same
 * grids, range, iso and min_weight); may be null when V = 0.                 */
int sfmhip_tsdf_integrate_colour(uint32_t* C, int D, int H, int W, int z0, int z1,
                                 const float* depth, const uint8_t* colour, int F, int Hd, int Wd,
                                 const float* poses, const float* Kf,
                                 const float* bmin, const float* bmax, float trunc,
                                 const float* table /* nullable */, void* stream);
int sfmhip_tsdf_surface_colours(const float* T, const float* Wt, const uint32_t* C,
                                int D, int H, int W, int z0, int z1, float iso, float min_weight,
                                const uint8_t* edge_mask, const int32_t* vert_off,
                                uint8_t* rgba /* [V][4] */, void* stream);

/* ---- V8: ray-cast of the fused TSDF grid (build-defined) -------------------
 * The depth map, normal map and colour image the fused model (T, Wt[, C])
 * predicts for V cameras: the third member of integrate / extract / ray-cast.
 * The reference has no counterpart (its sdf.py composites a learned SDF, V4).
 * Restated in numpy by tests/tsdf_raycast_ref.py.  Every f32 operation is one
 * IEEE round-to-nearest step in the order written, no FMA.
 *
 * Inputs: T, Wt (D,H,W) f32 as sfmhip_tsdf_integrate leaves them (D, H, W >= 2,
 * D*H*W < 2^31); C (D,H,W,4) u32 as V7 leaves it (nullable; 16-byte aligned);
 * poses [V][3][4] world->camera and Kf [V][4] = fx, fy, cx, cy (device f32);
 * image size Hd x Wd; HOST float[3] bmin / bmax (finite, |.| < 2^60, every
 * s_a = (bmax_a - bmin_a)/f32(R_a - 1) > 0; R = (W, H, D) for a = x, y, z); iso;
 * min_weight (<= 0 is SFMHIP_E_ARG); t_near >= 0, step > 0 (both finite) and
 * 1 <= n_samples <= 65536 (else SFMHIP_E_ARG).  V, Hd or Wd of 0: a no-op.
 * The call covers the whole grid: there is no z-range (a hit needs both samples
 * of a pair in the caller's grid; shard by views on a replicated grid).
 *
 * View skip rule (V5's): a view with a non-finite pose or intrinsic entry, or one
 * of magnitude >= 2^60, or with fx == 0 or fy == 0, gives all-zero outputs.
 *
 * Ray of pixel (v,u), pixel centres at integer coordinates (V5's convention);
 * Rra = poses[r][a], t_r = poses[r][3]:
 *   dc_x = (f32(u) - cx)/fx;  dc_y = (f32(v) - cy)/fy;  (dc_z = 1)
 *   o_a  = -((R0a t0 + R1a t1) + R2a t2)
 *   dw_a = (R0a dc_x + R1a dc_y) + R2a
 * The direction is not normalised: the ray parameter is the camera depth Zc.
 *
 * Point at parameter t:  p_a = o_a + t dw_a;  g_a = (p_a - bmin_a)/s_a;
 * i_a = floor(g_a);  f_a = g_a - i_a.  Its cell is IN RANGE iff
 * 0 <= i_a <= R_a - 2 on all three axes (a NaN fails) and VALID iff it is in
 * range and the 8 corner voxels (z,y,x) + {0,1}^3 are observed in V6's sense
 * (Wt >= min_weight and T finite).
 * Samples: t_k = t_near + f32(k) step, k = 0 .. n_samples-1 (no running sum).
 * F(k), for a VALID sample, with lerp(a,b,w) = a + w (b - a), Tzyx the corners:
 *   a_zy = lerp(T_zy0, T_zy1, f_x);  b_z = lerp(a_z0, a_z1, f_y);
 *   F = lerp(b_0, b_1, f_z).
 *
 * Hit: the smallest k in [1, n_samples) with samples k-1 and k both VALID,
 * F(k-1) >= iso and F(k) < iso: a front-face crossing (V6: inside(v) is
 * T < iso).  Back-face crossings and pairs with an invalid member are ignored
 * and the march goes on.  (A NaN F of a valid sample, from inf - inf of huge
 * finite corners, fails both comparisons.)
 *   depth = t_{k-1} + step ((F(k-1) - iso)/(F(k-1) - F(k)));  no hit: depth = 0,
 * V5's "invalid" value, so depth feeds sfmhip_tsdf_integrate as it is.
 *
 * Normal (nullable output, world frame) and colour (nullable, needs C) are taken
 * at p* = o + depth dw in p*'s own cell (i, f) by the rules above; both are all
 * zero when there is no hit or that cell is not VALID.
 *   Normal: the gradient of the cell's trilinear interpolant,
 *     x: d_zy = T_zy1 - T_zy0;  gx = lerp(lerp(d_00, d_01, f_y), lerp(d_10, d_11, f_y), f_z)/s_x
 *     y: d_zx = T_z1x - T_z0x;  gy = lerp(lerp(d_00, d_01, f_x), lerp(d_10, d_11, f_x), f_z)/s_y
 *     z: d_yx = T_1yx - T_0yx;  gz = lerp(lerp(d_00, d_01, f_x), lerp(d_10, d_11, f_x), f_y)/s_z
 *   len = sqrt((gx gx + gy gy) + gz gz); n = g/len, (0,0,0) when len is 0 or not
 *   finite.  It points towards increasing T, as V6's normals do.
 *   Colour: corner c = dx + 2 dy + 4 dz has weight w_c = (ux uy) uz with
 *   u_a = f_a where the corner's offset on axis a is 1, else 1 - f_a, and V7's mean
 *   col_c = f32(sum)/f32(n).  Starting from 0 and adding in ascending c over the
 *   corners with n > 0: num += w_c col_c (per channel), den += w_c; m = num/den;
 *   byte = rint(fmin(255, fmax(0, m))) half-even (fmin/fmax return the other
 *   operand for a NaN, so 0/0 gives 0), alpha 255.  No corner with n > 0:
 *   (0,0,0,0).
 *
 * Outputs (device): depth [V][Hd][Wd] f32; normals [V][Hd][Wd][3] f32; rgba
 * [V][Hd][Wd][4] u8 (4-byte aligned); steps [V][Hd][Wd] i32 (nullable,
 * diagnostic, outside the bit-exact contract): the number of samples whose F the
 * kernel evaluated for the pixel.
 *
 * Skipping (SFMHIP_RAYCAST_SKIP, default 1; 0 evaluates every sample of every
 * ray up to its hit): the kernel leaves out only samples it has proved cannot be
 * the k of a hit, and evaluates F(k-1) for the first k it keeps, so the outputs
 * are the plain march's bit for bit.  The proofs: (1) every operation from k to
 * i_a is monotone in k for a fixed ray, so i_a(k) is monotone and two samples in
 * one brick of 8^3 cells, or both outside the grid on the same side of one axis,
 * enclose only samples of that kind; (2) a valid sample whose cell origin lies in
 * a brick has its corners among the brick's voxels dilated by one (up), and with
 * L their minimum over the observed ones and A their largest magnitude,
 * A < 2^126, three nested lerps give F >= L - 20 2^-24 A - 2^-140 or NaN (each
 * lerp errs by at most 5.1 2^-24 max(|a|,|b|) + 2^-149 and the exact one stays in
 * [a,b]); a brick with L >= iso + (2^-19 A + 2^-126), or with no observed voxel,
 * cannot hold a sample with F < iso.  DESIGN.md K4d has the argument in full.   */
int sfmhip_tsdf_raycast(const float* T, const float* Wt, const uint32_t* C /* nullable */,
                        int D, int H, int W, const float* poses, const float* Kf, int V, int Hd, int Wd,
                        const float* bmin, const float* bmax, float iso, float min_weight,
                        float t_near, float step, int n_samples, float* depth,
                        float* normals /* nullable */, uint8_t* rgba /* nullable */,
                        int32_t* steps /* nullable */, void* stream);

/* ---- V9: frame-to-model tracking, point-to-plane ICP (build-defined) --------
 * Aligns a depth frame against the maps V8 renders of the model the frame is
 * about to be fused into: ray-cast, track, integrate is a closed loop on the
 * device.  The reference has no counterpart.  Restated in numpy by
 * tests/tsdf_track_ref.py.  Every f32 operation is one IEEE round-to-nearest step
 * in the order written, no FMA.  It uses V5's projection and V8's ray unchanged.
 *
 * Inputs (device f32), batched over B views, per view b: the frame depth_f
 * [B][Hf][Wf] with intrinsics Kf [B][4] = fx, fy, cx, cy; the current estimate
 * pose [B][3][4] world->camera (Rra = pose[r][a], t_r = pose[r][3]); the model
 * maps as V8 leaves them, depth_m [B][Hm][Wm] and normals_m [B][Hm][Wm][3] (world
 * frame, unit or all-zero), with their camera pose_m [B][3][4] (M below) and Km
 * [B][4] = fxm, fym, cxm, cym.  The two image sizes may differ (each below 2^20
 * per side and 2^31 pixels, B <= 65535).  Gates: dist2 > 0, the squared distance
 * limit; cos2 in [0, 1), the squared cosine limit, or any negative value to
 * switch the normal gate off.
 *
 * View skip rule (V5's): a non-finite entry or one of magnitude >= 2^60 in pose,
 * pose_m, Kf or Km, or fx, fy, fxm or fym of 0, gives zero sums for the view.
 *
 * Frame pixel (v,u), pixel centres at integer coordinates, d = depth_f[b][v][u]:
 * 1 Back-projection.  Reject unless d > 0 and d < 2^60 (a NaN fails: "the depth
 *   test").  pc = (((f32(u) - cx)/fx) d, ((f32(v) - cy)/fy) d, d);
 *   q_r = pc_r - t_r;  pw_a = (R0a q0 + R1a q1) + R2a q2.
 * 2 Association (V5's projection into the model camera).
 *   c_r = ((M_r0 pw_x + M_r1 pw_y) + M_r2 pw_z) + M_r3; reject unless
 *   2^-60 <= c_Z < 2^60; iz = 1/c_Z; um = floor((fxm c_X) iz + (cxm + 0.5)),
 *   vm = floor((fym c_Y) iz + (cym + 0.5)); reject unless 0 <= um < Wm and
 *   0 <= vm < Hm (a NaN fails).  dm = depth_m[b][vm][um]: reject unless dm > 0.
 *   nm = normals_m[b][vm][um]: reject when all three are 0 or one is not finite.
 * 3 Model vertex, by V8's ray of pixel (vm,um), so that a V8 depth gives back
 *   V8's hit point: dcx = (f32(um) - cxm)/fxm; dcy = (f32(vm) - cym)/fym;
 *   o_a = -((M0a M03 + M1a M13) + M2a M23);  dw_a = (M0a dcx + M1a dcy) + M2a;
 *   vmod_a = o_a + dm dw_a.
 * 4 Distance gate.  e_a = pw_a - vmod_a; accept iff
 *   (e_x e_x + e_y e_y) + e_z e_z <= dist2.
 * 5 Normal gate, only when cos2 >= 0 (no square root, no division: the mask is
 *   bit-exact).  The neighbours (v,u+1) and (v+1,u) must lie in the image and pass
 *   the depth test, else reject.  With pc' of the right and pc" of the lower
 *   neighbour (step 1's formula): a = pc' - pc, bv = pc" - pc,
 *   c = bv x a = (bv_y a_z - bv_z a_y, bv_z a_x - bv_x a_z, bv_x a_y - bv_y a_x)
 *   (two products and one subtraction each),
 *   cw_a = (R0a c0 + R1a c1) + R2a c2,  dotr = (cw_x nm_x + cw_y nm_y) + cw_z nm_z,
 *   cc = (cw_x cw_x + cw_y cw_y) + cw_z cw_z.  In camera coordinates c points
 *   towards the camera iff fx fy > 0; a mirrored frame (exactly one of fx, fy
 *   negative, which V5 and V8 accept) turns it round, so
 *   dotv = -dotr when (fx < 0) != (fy < 0), else dotr: an exact sign change, cc is
 *   the same either way.  The sign of det R does not enter: cw = R^T c is c in
 *   world coordinates for any orthogonal R.  Accept iff dotv > 0 and
 *   dotv dotv >= cos2 cc.
 * 6 Row.  r = (nm_x e_x + nm_y e_y) + nm_z e_z;  J = (pw x nm, nm), six f32, the
 *   cross product written as in step 5.
 *
 * Sums (f64) over the accepted pixels of a view, 29 doubles, sums [B][29]:
 *   [0..20] A_ij = sum f64(J_i) f64(J_j), i <= j, upper triangle row-major;
 *   [21..26] g_i = sum f64(J_i) f64(r);  [27] E = sum f64(r)^2;  [28] n, the count.
 * Every product of two f32 is exact in f64, so only the order of the additions is
 * implementation-defined; it is a fixed function of the shapes (no floating-point
 * atomics, nothing depends on the CU count or the dispatch order): two runs give
 * the same bits on any device.  The order: 16 x 16 pixel tiles in row-major order,
 * nt of them; a workgroup takes share = max(4, ceil(nt/1024)) consecutive tiles; a
 * pixel's lane is 8 (v mod 8) + (u mod 8) of wave 2 ((v mod 16) div 8) +
 * ((u mod 16) div 8); a lane adds its pixels in tile order, the 64 lanes of a
 * wave are added by the binary tree x_l += x_(l + off), off = 32, 16, .. 1, the 4
 * waves in order, and the P workgroups' partials in 32 runs of ceil(P/32)
 * consecutive ones, each run in order, then the runs in order.
 * mask (nullable) [B][Hf][Wf] u8: 1 where the pixel was accepted, else 0.
 *
 * Solve and update (f64, per view), delta = (omega, v) with A delta = -g by LDL^T
 * without pivoting (d_j = A_jj - sum_(m<j) (L_jm L_jm) d_m).  The view is LOST when
 * n < min_pairs or a pivot is not above 1e-12 trace(A): its pose stays as it is,
 * bit for bit, and its later iterations are no-ops (their log records carry zero
 * sums and delta and the status).  A view taken out by the skip rule has zero
 * sums, is lost too, and carries status 2.  Otherwise dR = Rodrigues(omega)
 * (theta = |omega|, k = omega/theta, dR = cos(theta) I + (1 - cos(theta)) k k^T +
 * sin(theta) [k]x; I when theta = 0), R' = R dR^T, t' = t - R' v: the world-frame
 * increment pw <- dR pw + v applied to the world->camera pose.  The pose is
 * carried in f64 across the iterations of one call; each iteration's per-pixel
 * arithmetic reads its f32 rounding.
 *
 * sfmhip_icp_normal_equations: one linearisation at the given poses.
 * sfmhip_icp_track: n_iters iterations (2 n_iters plain kernel launches on the
 * stream, no host round trip); pose_inout [B][3][4] f32 device; log (nullable,
 * device) [B][n_iters][36] f64: the 29 sums, the 6 delta, the status (0 ok,
 * 1 lost, 2 skipped view).
 * B, Hf Wf or n_iters of 0: a no-op.  dist2 <= 0, cos2 >= 1 (or either NaN),
 * min_pairs < 6: SFMHIP_E_ARG.  An empty model image (Hm Wm = 0, the model maps
 * may be null) with a non-empty frame is valid and gives lost views.  Both calls
 * are asynchronous on the stream; scratch comes from the library pool.           */
int sfmhip_icp_normal_equations(const float* depth_f, const float* Kf, const float* pose, int B, int Hf, int Wf,
                                const float* depth_m, const float* normals_m, const float* pose_m,
                                const float* Km, int Hm, int Wm, float dist2, float cos2,
                                double* sums, uint8_t* mask /* nullable */, void* stream);
int sfmhip_icp_track(const float* depth_f, const float* Kf, int B, int Hf, int Wf,
                     const float* depth_m, const float* normals_m, const float* pose_m,
                     const float* Km, int Hm, int Wm, float dist2, float cos2,
                     int n_iters, int min_pairs, float* pose_inout, double* log /* nullable */,
                     void* stream);

/* ---- V10: dense depth from posed images, census plane-sweep stereo (build-defined)
 * Multi-view stereo: V posed grey images in, one depth map per reference view out,
 * in the conventions of V5 (0 = invalid), so the maps feed sfmhip_tsdf_integrate as
 * they are.  The reference has no counterpart.  Restated in numpy by
 * tests/mvs_ref.py.  The costs are integers; every f32 operation is one IEEE
 * round-to-nearest step in the order written, no FMA: every output is defined to
 * the bit.
 *
 * Views: one size (H, W) for all; img [V][H][W] u8; poses [V][3][4] f32
 * world->camera; K [V][4] = fx, fy, cx, cy; pixel centres at integer coordinates.
 * View skip rule (V5's): a non-finite entry or one of magnitude >= 2^60 in a
 * view's pose or intrinsics, or fx or fy of 0, makes the view invalid.  An invalid
 * reference (or a refs entry outside [0, V)) gives all-zero outputs; an invalid
 * source, a srcs entry of -1 ("none") or one outside [0, V) is out of view
 * everywhere.
 *
 * 1 Census (sfmhip_census), cen [V][H][W] u64, 7 x 7: for (dy, dx) from (-3, -3) to
 *   (3, 3) in row-major order without the centre, bit i (i = 0..47 in that order)
 *   is 1 iff the neighbour lies inside the image and img[nb] > img[centre]; bits
 *   48..63 are 0.
 * 2 Relative pose per (reference r, source s), in f64 from the f32 entries:
 *   Rrel[i][j] = (Rs[i][0] Rr[j][0] + Rs[i][1] Rr[j][1]) + Rs[i][2] Rr[j][2];
 *   trel[i] = ts[i] - ((Rrel[i][0] tr[0] + Rrel[i][1] tr[1]) + Rrel[i][2] tr[2]) with
 *   the f64 Rrel; both then rounded to f32 (R, t below).
 * 3 Raw cost of reference pixel (v, u), plane depth z = planes[k], source s (f32):
 *   dx = (f32(u) - cx)/fx; dy = (f32(v) - cy)/fy (V8's ray); X = dx z; Y = dy z;
 *   xc = ((R00 X + R01 Y) + R02 z) + t0, yc and zc by rows 1 and 2; visible requires
 *   2^-60 <= zc < 2^60; iz = 1/zc; pu = floor((fx_s xc) iz + (cx_s + 0.5)),
 *   pv = floor((fy_s yc) iz + (cy_s + 0.5)) (V5's rule); visible also requires
 *   0 <= pu < W and 0 <= pv < H (a NaN fails).  Visible: c = popcount(cen[r][v][u] ^
 *   cen[s][pv][pu]); not visible: c = penalty.  raw[k][v][u] = sum_s c over all S
 *   entries of the reference's source list; nv[k][v][u] = the number of visible ones.
 * 4 Aggregation: ag[k][v][u] = the sum of raw[k] over the (2a+1)^2 window around
 *   (v, u); a window position outside the image contributes penalty S.  int32.
 * 5 Winner: k* = the smallest k attaining min_k ag; best = ag[k*]; second = the
 *   minimum of ag[k] over |k - k*| >= 2, or INT32_MAX if there is none.
 * 6 Sub-plane depth: inv[k] = 1/planes[k] (an f32 division); c0, cm, cp = ag at k*,
 *   k* - 1, k* + 1 as f32; den = (cm - c0) + (cp - c0); off = (cm - cp)/(2 den) if
 *   0 < k* < P - 1 and den > 0, else 0; step = inv[k*+1] - inv[k*] if off >= 0, else
 *   inv[k*] - inv[k*-1]; depth = 1/(inv[k*] + off step).
 * 7 Validity: depth = 0 unless 0 < k* < P - 1, nv[k*][v][u] >= min_views and
 *   256 best <= uniq second (compared in int64; uniq in 0..256, 256 disables it).
 * 8 Consistency (sfmhip_depth_consistency): for reference r with d_r = depth[r] and
 *   each source s of its list, from the same array depth [V][H][W]: a pixel with
 *   d_r > 0 is reprojected exactly as in step 3 with z = d_r; the source is
 *   consistent iff the pixel is visible, ds = depth[s][pv][pu] > 0 and
 *   fabsf(ds - zc) <= eps zc.  count [R][H][W] u8 = the number of consistent
 *   sources (0 where d_r is not > 0); filtered [R][H][W] = d_r where d_r > 0 and
 *   count >= min_consistent, else 0.  depth and filtered must not overlap.
 *
 * Limits: 1 <= S <= 16, 0 <= a = agg_radius <= 3, 0 <= penalty <= 48, 1 <= P <= 65535,
 * 0 <= uniq <= 256, min_views >= 0, eps finite and >= 0, min_consistent >= 0,
 * R <= 65535, H and W below 2^20 and H W below 2^31: otherwise SFMHIP_E_ARG, like a
 * null pointer, without touching the GPU.  ag <= 48 49 16 < 2^16, so (ag << 16) | k
 * is a u32 key whose minimum is the winner with the tie rule built in.  P < 3 is
 * legal and gives all-invalid maps.  planes [P] must be finite, positive and
 * strictly monotonic in either direction: they are device memory, so this is the
 * caller's duty (the Python wrapper checks it); the steps above are defined for any
 * values.  R = 0 or H W = 0 (V = 0 or H W = 0 for the census) is a no-op without a
 * launch.
 *
 * All arrays are device memory: refs [R] i32, srcs [R][S] i32, planes [P] f32;
 * outputs depth [R][H][W] f32 and the nullable diagnostics kstar [R][H][W] i32,
 * best, second (i32) and nv (u8) = nv[k*].  The calls are asynchronous plain
 * launches on the stream; scratch comes from the library pool.  No atomics: two
 * runs give the same bits.
 *
 * Semi-global smoothing (optional; sfmhip_cost_volume, sfmhip_sgm_aggregate,
 * sfmhip_volume_select; restated by tests/mvs_sgm_ref.py).  Between steps 4 and 5:
 * 4a Cost volume: vol[r][v][u][k] = ag[k][v][u] of step 4 as u16 (ag <= 37632), the
 *   plane index innermost.  An invalid reference gives an all-zero slice.
 * 4b Path aggregation with integers 0 <= p1 <= p2 <= 16383 and a non-zero 8-bit
 *   path_mask whose bit i selects the direction d_i = (dv, du) of (0,+1), (0,-1),
 *   (+1,0), (-1,0), (+1,+1), (+1,-1), (-1,+1), (-1,-1).  For a selected d, pixel
 *   p = (v, u) and predecessor q = p - d: L_d(p, k) = vol(p, k) if q lies outside
 *   the image; otherwise, with m = min_j L_d(q, j),
 *   L_d(p, k) = vol(p, k) + min(L_d(q, k), L_d(q, k-1) + p1 [only if k > 0],
 *   L_d(q, k+1) + p1 [only if k < P-1], m + p2) - m.  So vol <= L_d <= vol + p2 < 2^16.
 *   sm[r][v][u][k] = the sum of L_d(p, k) over the selected d, u32, below 2^19.
 * 5'-7' Selection: steps 5, 6 and 7 as written with sm in place of ag (the smallest
 *   k of the minimum; second over |k - k*| >= 2 or INT32_MAX; the same f32 parabola;
 *   256 best <= uniq second in int64).  nv stays step 3's count at planes[k*]; it
 *   does not depend on the smoothing.  An invalid reference gives all-zero outputs.
 * Limits of this mode: 1 <= P <= 256 for sfmhip_sgm_aggregate and
 * sfmhip_volume_select; p1 > p2, p2 > 16383 or path_mask outside [1, 255] is
 * SFMHIP_E_ARG, like a null pointer and the limits above, without touching the
 * GPU; R = 0 or H W = 0 is a no-op without a launch.  sfmhip_sgm_aggregate takes no
 * cameras and is defined for any u16 volume; sfmhip_volume_select is defined for
 * sm entries below 2^24.  sm must not overlap vol.  Plain asynchronous launches on
 * the stream (one per selected direction: the first writes sm, the others add to
 * it, no atomics); two runs give the same bits.                                  */
int sfmhip_cost_volume(const uint64_t* cen, const float* poses, const float* K, int V, int H, int W,
                       const int32_t* refs, const int32_t* srcs, int R, int S,
                       const float* planes, int P, int agg_radius, int penalty,
                       uint16_t* vol /* [R][H][W][P] */, void* stream);
int sfmhip_sgm_aggregate(const uint16_t* vol, int R, int H, int W, int P, int p1, int p2, int path_mask,
                         uint32_t* sm /* [R][H][W][P] */, void* stream);
int sfmhip_volume_select(const uint32_t* sm, const float* poses, const float* K, int V, int H, int W,
                         const int32_t* refs, const int32_t* srcs, int R, int S,
                         const float* planes, int P, int uniq, int min_views,
                         float* depth, int32_t* kstar /* nullable */, int32_t* best /* nullable */,
                         int32_t* second /* nullable */, uint8_t* nv /* nullable */, void* stream);
int sfmhip_census(const uint8_t* img, int V, int H, int W, uint64_t* cen, void* stream);
int sfmhip_plane_sweep(const uint64_t* cen, const float* poses, const float* K, int V, int H, int W,
                       const int32_t* refs, const int32_t* srcs, int R, int S,
                       const float* planes, int P, int agg_radius, int penalty, int uniq, int min_views,
                       float* depth, int32_t* kstar /* nullable */, int32_t* best /* nullable */,
                       int32_t* second /* nullable */, uint8_t* nv /* nullable */, void* stream);
int sfmhip_depth_consistency(const float* depth, const float* poses, const float* K, int V, int H, int W,
                             const int32_t* refs, const int32_t* srcs, int R, int S, float eps,
                             int min_consistent, uint8_t* count, float* filtered, void* stream);

/* ---- V12: undistortion of images and depth maps for the dense path (build-defined)
 * V10 and V5 - V9 take pinhole cameras.  These calls resample V views seen through the
 * radial model of the calibrating bundle adjustment (sfmhip_ba_calib) to pinhole
 * views, a gather per output pixel.  The reference has no counterpart.  Restated in
 * numpy by tests/undistort_ref.py.  The map is f64, one IEEE round-to-nearest step per
 * operation in the order written, no FMA; the blend is integer: every output is
 * defined to the bit.
 *
 * Cameras (device memory): cam_src [V][6] f64 = fx, fy, cx, cy, k1, k2 (OpenCV's radial
 * model with p1 = p2 = k3 = 0) of the source images [V][H][W]; cam_dst [V][4] f64 =
 * gx, gy, ox, oy, the pinhole camera of the outputs [V][Ho][Wo].  Pixel centres at
 * integer coordinates.  View skip rule: a non-finite number among the 10 of a view,
 * one of magnitude >= 2^60, or fx, fy, gx or gy of 0 makes every output pixel of the
 * view invalid.
 *
 * The map of output pixel (u, v):
 *   x = (u - ox) / gx;  y = (v - oy) / gy;  r2 = x x + y y;  r4 = r2 r2;
 *   d = (1 + k1 r2) + k2 r4;  mono = (1 + (3 k1) r2) + (5 k2) r4   (the derivative of
 *   r d(r): positive where the model has not folded over);
 *   sx = (d x) fx + cx;  sy = (d y) fy + cy;
 *   fin = mono > 0 and |sx| < 2^30 and |sy| < 2^30 (a NaN fails);
 *   X = floor(sx 256 + 0.5), Y = floor(sy 256 + 0.5): integers, units of 1/256 px;
 *   valid = fin and 0 <= X <= (W - 1) 256 and 0 <= Y <= (H - 1) 256.
 * Validity is decided on the rounded X, Y: a source coordinate that misses the border
 * by less than 1/512 px is inside.
 *
 * sfmhip_undistort_map: map [V][Ho][Wo][2] i32 = X, Y, or -1, -1 where invalid (8-byte
 *   aligned).  Takes no image: H, W only bound X, Y.
 * sfmhip_undistort_u8 (bilinear; C = 1, 3 or 4 interleaved channels, all alike):
 *   x0 = X >> 8, a = X & 255, x1 = min(x0 + 1, W - 1); y0, b, y1 likewise from Y;
 *   out = ((256-a)(256-b) p[y0][x0] + a (256-b) p[y0][x1] + (256-a) b p[y1][x0]
 *          + a b p[y1][x1] + 32768) >> 16   (exact in u32);
 *   mask [V][Ho][Wo] u8 = 1.  An invalid pixel: 0 in every channel and in the mask.
 * sfmhip_undistort_f32 (nearest; for depth maps, whose z is unchanged by a radial
 *   model and where 0 = invalid): the 32 bits of
 *   src[min((Y + 128) >> 8, H - 1)][min((X + 128) >> 8, W - 1)], copied as they are (no
 *   blending: no depth is invented across an edge); an invalid pixel: 0.
 *
 * Limits: V <= 65535; H, W, Ho, Wo <= 32768; C of 1, 3 or 4; dst 4-byte aligned when
 * C = 4 and map 8-byte aligned: otherwise SFMHIP_E_ARG, like a null pointer, without
 * touching the GPU.  V = 0, Ho Wo = 0, or for the two
 * resampling calls H W = 0, is a no-op without a launch.  dst must not overlap src.
 * Asynchronous plain launches on the stream (the x of every column and the y of every
 * row of a view first, in scratch from the library pool; then one lane per output
 * pixel); no atomics: two runs give the same bits.                                  */
int sfmhip_undistort_u8(const uint8_t* src, int V, int H, int W, int C, const double* cam_src,
                        const double* cam_dst, int Ho, int Wo, uint8_t* dst /* [V][Ho][Wo][C] */,
                        uint8_t* mask /* [V][Ho][Wo] */, void* stream);
int sfmhip_undistort_f32(const float* src, int V, int H, int W, const double* cam_src, const double* cam_dst,
                         int Ho, int Wo, float* dst /* [V][Ho][Wo] */, void* stream);
int sfmhip_undistort_map(const double* cam_src, const double* cam_dst, int V, int H, int W, int Ho, int Wo,
                         int32_t* map /* [V][Ho][Wo][2] */, void* stream);

/* ---- V13: planning the dense stage from a sparse reconstruction (build-defined)
 * V10 takes source lists and depth planes, V5 a box: these calls derive them from the
 * cameras, points and observations of a reconstruction (plan.py: view selection, depth
 * ranges, scene bounds).  The reference has no counterpart.  Restated in numpy by
 * tests/plan_ref.py.  f64 arithmetic, one IEEE round-to-nearest step per operation in
 * the order written, no FMA; every sum is an integer sum (integer atomics): every
 * output is defined to the bit and does not depend on the launch geometry.  All
 * pointers are device memory.
 *
 * sfmhip_obs_depth: the camera-frame depth of M observations.  poses [V][3][4] f64
 *   world -> camera, X [N][3] f64, obs_cam / obs_pt [M] i32.  With P = poses[obs_cam[m]]
 *   and x = X[obs_pt[m]]:
 *     d = ((P[2][0] x0 + P[2][1] x1) + P[2][2] x2) + P[2][3];  z[m] = f32(d);
 *   where f32(d) is not finite or not > 0 (a NaN, a point behind the camera, an f64
 *   depth that overflows or underflows f32), z[m] = +inf: it sorts last and is not
 *   counted.  One lane per observation.  Every index must lie in [0, V) x [0, N): the
 *   lists live on the device, so the wrapper (plan.py) checks them on the host before
 *   the call and raises without a launch; the kernel reads nothing out of bounds for an
 *   index that does not (such an observation gets +inf).  M <= 2^38.
 *
 * sfmhip_view_pair_counts: for every pair of views, the tracks both observe and those
 *   among them with a usable triangulation angle.  centres [V][3] f64 (the wrapper's
 *   c_i = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2), f64 on the host); X [N][3] f64;
 *   obs_cam [M] i32 sorted by (point, camera) with pt_off [N+1] i64, the layout of
 *   sfmhip_ba_global*, every (camera, point) pair at most once (the wrapper removes
 *   repeats); c2_lo = cos^2 of the largest angle, c2_hi = cos^2 of the smallest, the
 *   largest at most 90 degrees: 0 <= c2_lo <= c2_hi <= 1, else SFMHIP_E_ARG.
 *   For a track x seen by cameras a and b, a != b:
 *     ra = c_a - x;  rb = c_b - x  (per component);
 *     d = (ra0 rb0 + ra1 rb1) + ra2 rb2;
 *     n = ((ra0 ra0 + ra1 ra1) + ra2 ra2) ((rb0 rb0 + rb1 rb1) + rb2 rb2);
 *     good iff d > 0 and n < inf and d d >= c2_lo n and d d <= c2_hi n.
 *   shared [V][V] i32: the tracks both views observe; good [V][V] i32: those that are
 *   good; both symmetric with a zero diagonal, overwritten.  A point on a camera centre
 *   (d = 0) and a point with a NaN are shared and not good by the comparisons alone;
 *   `n < inf` makes that hold for an infinite coordinate too (inf >= inf would pass).
 *   A track whose range in pt_off is not inside [0, M], is reversed or is longer than V
 *   is skipped, like a camera index outside [0, V).  V <= 32767.  V = 0 is a no-op;
 *   M = 0, N = 0 or V = 1 zero the outputs without a launch.
 *   A track of length L has L (L - 1) / 2 pairs; the pairs, not the tracks, are dealt
 *   out evenly over the lanes of a workgroup.  While 4 V (V - 1) bytes fit the 160 KiB of
 *   LDS beside 3136 bytes of bookkeeping (V <= 200) every workgroup counts into upper
 *   triangles of its own in LDS and adds its non-zero entries to global memory once;
 *   above that, or under SFMHIP_PLAN_GLOBAL=1, every pair adds straight to global
 *   memory.  Integer sums: both paths give the same bits.
 *
 * sfmhip_segmented_select: exact order statistics of f32 values per segment.  values
 *   [M] f32, seg_off [S+1] i64 (segment s = values[seg_off[s] .. seg_off[s+1])), ranks
 *   [S][R] i64, out [S][R] f32, R <= 8.  Total order: that of the radix key of the 32
 *   bits, key = ~bits for a set sign bit, else bits ^ 0x80000000: -0.0 < +0.0, +inf
 *   and the NaNs with a clear sign bit last.  out[s][r] = the value whose key has rank
 *   ranks[s][r] (0 = smallest) among the n_s keys of segment s, its 32 bits as they are;
 *   equal keys are equal values, so ties need no rule.  A rank outside [0, n_s) gives
 *   the quiet NaN 0x7FC00000; a segment not inside [0, M] or reversed is empty.  One
 *   workgroup per segment, four 8-bit most-significant-digit passes with LDS
 *   histograms; the segment is not sorted and nothing returns to the host.
 *
 * A null pointer or a negative size is SFMHIP_E_ARG; shapes are checked before the
 * empty-call no-op (M = 0 for obs_depth; S = 0 or R = 0 for the select).  Asynchronous
 * on the stream.                                                                       */
int sfmhip_obs_depth(const double* poses, int V, const double* X, int64_t N, const int32_t* obs_cam,
                     const int32_t* obs_pt, int64_t M, float* z /* [M] */, void* stream);
int sfmhip_view_pair_counts(const double* centres, int V, const double* X, int64_t N, const int32_t* obs_cam,
                            int64_t M, const int64_t* pt_off, double c2_lo, double c2_hi,
                            int32_t* shared /* [V][V] */, int32_t* good /* [V][V] */, void* stream);
int sfmhip_segmented_select(const float* values, int64_t M, const int64_t* seg_off, int64_t S,
                            const int64_t* ranks, int R, float* out /* [S][R] */, void* stream);

/* ---- V11: SIFT keypoints and descriptors (build-defined) ---------------------
 * Scale-space extrema, orientation and the 128-d descriptor of V grey images, in
 * four calls.  The reference has no counterpart (it reads features from disk).
 * Restated in numpy by tests/sift_ref.py.  V10's rule holds: every f32 operation
 * is one IEEE round-to-nearest step in the order written, no FMA; sqrt and / are
 * correctly rounded; sums of floats have the order written; no floating-point
 * atomics: every output is defined to the bit and two runs give the same bits.
 * No device exp / atan2 / cos: Gaussian taps, window tables and the cos/sin table
 * are inputs (built in f64 on the host and rounded to f32; features.sift_tables()),
 * the angle is the polynomial turn() below.
 *
 * Constants: S = 3 intervals, L = S + 3 = 6 Gaussian levels and S + 2 DoG levels per
 * octave, O octaves (1 <= O <= 16, min(H, W) >> (O - 1) >= 1).  Octave o has
 * H_o = ((H - 1) >> o) + 1 rows and W_o = ((W - 1) >> o) + 1 columns (octave 0 is the
 * image: no doubling).  Pixel centres are at integer coordinates.
 *
 * Pyramid buffer pyr [V][per] f32 with per = L sum_o H_o W_o: level s of octave o of
 * view v starts at v per + off_o + s H_o W_o, off_o = L sum_{j<o} H_j W_j, row-major.
 *
 * 1 Pyramid (sfmhip_sift_pyramid).  taps [L][27] f32 (device): row s holds the
 *   2 r_s + 1 taps of blur s, the rest of the row is unused; radii [L] i32 is HOST
 *   memory, 0 <= r_s <= 13.  blur(src, s): rows first, tmp[y][x] = acc after
 *   acc = 0; for k = 0 .. 2r: acc = acc + tap[k] src[y][clamp(x + k - r, 0, W_o - 1)];
 *   then columns, dst[y][x] likewise over tmp[clamp(y + k - r, 0, H_o - 1)][x].
 *   Level 0 of octave 0 = blur(f32(img), 0); level s = blur(level s - 1, s);
 *   level 0 of octave o + 1 = level S of octave o at rows 2y and columns 2x.
 *   (The wrapper's taps: sig[s] = 1.6 2^(s/S); blur 0 has sigma sqrt(sig[0]^2 - 0.25),
 *   blur s sqrt(sig[s]^2 - sig[s-1]^2); r = ceil(4 sigma); exp(-k^2 / (2 sigma^2))
 *   normalised to sum 1 in f64.)
 *
 * 2 Detect (sfmhip_sift_detect).  D(l, y, x) = G[l+1][y][x] - G[l][y][x], formed on
 *   the fly.  A sample (o, l, y, x) with 1 <= l <= S, border <= y <= H_o - 1 - border,
 *   border <= x <= W_o - 1 - border starts a candidate iff |D| > prethresh and D is
 *   strictly greater than all 26 neighbours in (l, y, x) or strictly less than all.
 *   Refinement, at most 5 times at the current integer (l, y, x), with D.. = D there:
 *     gx = (D(x+1) - D(x-1)) 0.5, gy and gl likewise along y and l;
 *     c2 = 2 D; hxx = (D(x+1) + D(x-1)) - c2, hyy and hll likewise;
 *     hxy = ((D(y+1,x+1) - D(y+1,x-1)) - (D(y-1,x+1) - D(y-1,x-1))) 0.25, hxl with
 *     (l, x) and hyl with (l, y) in the places of (y, x);
 *     A00 = hyy hll - hyl hyl; A01 = hxl hyl - hxy hll; A02 = hxy hyl - hxl hyy;
 *     A11 = hxx hll - hxl hxl; A12 = hxy hxl - hxx hyl; A22 = hxx hyy - hxy hxy;
 *     det = (hxx A00 + hxy A01) + hxl A02; reject unless |det| > 0 (NaN rejects);
 *     ox = -(((A00 gx + A01 gy) + A02 gl) / det); oy = -(((A01 gx + A11 gy) + A12 gl) / det);
 *     ol = -(((A02 gx + A12 gy) + A22 gl) / det);
 *     converged iff |ox| < 0.5, |oy| < 0.5 and |ol| < 0.5: stop.  Otherwise reject
 *     unless all three are <= 1048576 in magnitude (NaN rejects), move by
 *     (rint(ol), rint(oy), rint(ox)) and reject if the new sample violates the
 *     bounds of a start sample.  Not converged after the 5th solve: reject.
 *   At the converged sample: resp = D + 0.5 ((gx ox + gy oy) + gl ol); reject if
 *   |resp| 3.0 < contrast_thr (the wrapper passes f32(contrast 255)); tr = hxx + hyy;
 *   d2 = hxx hyy - hxy hxy; reject if d2 <= 0 or (tr tr) edge_r >= ((edge_r + 1)
 *   (edge_r + 1)) d2 (a NaN on either side rejects).  The scale in octave pixels,
 *   from sig [L] f32 (device): sc = sig[l] + ol (sig[l+1] - sig[l]) if ol >= 0, else
 *   sig[l] + ol (sig[l] - sig[l-1]).
 *   Record, 8 32-bit words: octave (i32), level l (i32; the converged one),
 *   x = f32(x) + ox, y = f32(y) + oy, sc, |resp|, x 2^o, y 2^o (f32).
 *   Output rec [V][cap][8] in ascending (octave, level, row, column) of the START
 *   sample; count [V] i32 holds the true total; only the first cap records are
 *   written, the rest of rec stays untouched.  Count, scan, write; no atomics.
 *
 * turn(y, x) in turns, in [0, 1): a = |x|, b = |y|, m = max(a, b), t = min(a, b) / m
 *   (0 if m == 0); u = t t; p = ((((C4 u + C3) u + C2) u + C1) u + C0) t with C0..C4 =
 *   0x1.45e8e8p-3, -0x1.aec82ap-5, 0x1.d67172p-6, -0x1.bd6ba4p-7, 0x1.b4a748p-9;
 *   if b > a: p = 0.25 - p; if signbit(x): p = 0.5 - p; if signbit(y): p = 1 - p;
 *   if p >= 1: p = 0.  Within 2^-18 turn of atan2 (tests/test_sift_cpu.py).
 *
 * sample(G, px, py), bilinear with clamped indices, G one level (H_o x W_o):
 *   x0 = floor(px); fx = px - x0; i0 = clamp(int(min(max(x0, -1), W_o)), 0, W_o - 1),
 *   i1 = clamp(int(min(max(x0, -1), W_o)) + 1, 0, W_o - 1) (min/max as fminf/fmaxf);
 *   y0, fy, j0, j1 likewise; top = G[j0][i0] (1 - fx) + G[j0][i1] fx, bot with j1;
 *   value = top (1 - fy) + bot fy.
 *
 * 3 Orient (sfmhip_sift_orient), per record k < min(count[v], cap), on level l of
 *   its octave: h = (sc 4.5) 0.125; P[i][j] = sample(x + f32(j - 9) h, y + f32(i - 9) h),
 *   i, j = 0..18.  For i, j = 1..17: gx = P[i][j+1] - P[i][j-1]; gy = P[i+1][j] -
 *   P[i-1][j]; w = sqrt(gx gx + gy gy) wo[i-1][j-1] (wo [17][17] f32, device; the
 *   wrapper's Gaussian of sigma 1.5 sc = 8/3 samples); bin = min(int(floor(turn(gy,
 *   gx) 36)), 35); the histogram is an INTEGER sum: hist[bin] += int(rint(min(w 1024,
 *   4194304))) in i32 (fminf: a NaN counts as the bound).  As f32 it is smoothed
 *   twice: h'[b] = (h[b-1] + h[b+1]) 0.25 + h[b] 0.5, circular.  With M its maximum,
 *   bin b is a peak iff h[b] > h[b-1], h[b] > h[b+1] and h[b] >= 0.8 M; its
 *   orientation is q = int(rint(((f32(b) + 0.5 + 0.5 (h[b-1] - h[b+1]) / ((h[b-1] - 2
 *   h[b]) + h[b+1])) 1024) / 36)) mod 1024, in units of 1/1024 turn.  The first 4 peaks
 *   in ascending bin order give one oriented record each: the record with word 1
 *   replaced by l | (q << 8).  Output orec [V][cap_o][8], records in input order;
 *   ocount [V] the true total, the first cap_o written, the rest untouched.
 *
 * 4 Describe (sfmhip_sift_describe), per oriented record k < min(ocount[v], cap_o):
 *   (c, s) = cs[q] (cs [1024][2] f32, device: cos and sin of q/1024 turn);
 *   h = (sc 12) 0.0625; u = f32(j) - 8.5, v = f32(i) - 8.5, P[i][j] = sample(x + ((u c)
 *   - (v s)) h, y + ((u s) + (v c)) h), i, j = 0..17.  For i, j = 1..16 (a = i - 1,
 *   b = j - 1): gx, gy as in step 3; m = sqrt(gx gx + gy gy) wd[a][b] (wd [16][16]
 *   f32, device: Gaussian of sigma 8 samples about (7.5, 7.5)); ob = turn(gy, gx) 8;
 *   o0 = floor(ob); fo = ob - o0; orientation bins int(o0) mod 8 with weight 1 - fo
 *   and (int(o0) + 1) mod 8 with weight fo.  cw [4][16] f32 (device): cw[k][a] =
 *   max(0, 1 - |(a - 1.5)/4 - k|), the bilinear weight of sample a in cell k.  Bin
 *   (ky, kx, o), index (ky 4 + kx) 8 + o: d = the sum, added in row-major order of
 *   (a, b) from 0, of ((m cw[ky][a]) cw[kx][b]) wgt_o(a, b); terms that are 0 may be
 *   skipped.  n = sqrt(sum_{bin ascending} d d) (acc = acc + d d from 0); all-zero
 *   output unless n > 0; e = min(d / n, 0.2); n' likewise over e;
 *   desc[bin] = u8(min(rint(512 (e / n')), 255)).  Output desc [V][cap_o][128] u8;
 *   rows at and beyond min(ocount[v], cap_o) stay untouched.
 *
 * Limits: 1 <= O <= 16 with min(H, W) >> (O - 1) >= 1, H W < 2^31, 0 <= V <= 65535,
 * cap >= 0, cap_o >= 0, V cap and V cap_o below 2^28 (2^24 for the descriptors),
 * border >= 1, radii in [0, 13]: otherwise SFMHIP_E_ARG, like a null
 * pointer, without touching the GPU.  V = 0 is a no-op without a launch; cap = 0
 * still counts.  An octave with H_o or W_o < 2 border + 1 holds no start sample.
 * Records handed to steps 3 and 4 must have 0 <= octave < O, 1 <= l <= S (l = word 1
 * mod 256), finite x, y and sc with |x| <= 1048576, |y| <= 1048576 and 0 < sc <= 1048576
 * (what step 2 writes).  A record outside that contract reads nothing: it yields no
 * oriented record from step 3 (it counts 0 peaks) and an all-zero descriptor row from
 * step 4.  rec, orec, the tables and pyr are device memory.
 * Plain asynchronous launches on the stream; scratch from the library pool.       */
int sfmhip_sift_pyramid(const uint8_t* img, int V, int H, int W, int O, const float* taps /* [6][27] */,
                        const int32_t* radii /* HOST [6] */, float* pyr, void* stream);
int sfmhip_sift_detect(const float* pyr, int V, int H, int W, int O, const float* sig /* [6] */, int border,
                       float prethresh, float contrast_thr, float edge_r, int cap,
                       int32_t* rec /* [V][cap][8] */, int32_t* count /* [V] */, void* stream);
int sfmhip_sift_orient(const float* pyr, int V, int H, int W, int O, const int32_t* rec, const int32_t* count,
                       int cap, const float* wo /* [17][17] */, int cap_o, int32_t* orec /* [V][cap_o][8] */,
                       int32_t* ocount /* [V] */, void* stream);
int sfmhip_sift_describe(const float* pyr, int V, int H, int W, int O, const int32_t* orec,
                         const int32_t* ocount, int cap_o, const float* wd /* [16][16] */,
                         const float* cw /* [4][16] */, const float* cs /* [1024][2] */,
                         uint8_t* desc /* [V][cap_o][128] */, void* stream);

/* ---- §8f row 2: geometric verification (batched over image pairs) --------
 * cv2.findEssentialMat(pts0, pts1, K, method=cv2.RANSAC, prob=0.999,
 * threshold=1) at matching.py:134 and sfm.py:108 (OpenCV five-point.cpp +
 * ptsetreg.cpp, maxIters 1000 by default): cv::RNG(-1) 5-point samples,
 * Nister solver, Sampson error (float) <= (thresh/((fx+fy)/2))^2, a model
 * replaces the best iff count > max(best, 4), RANSACUpdateNumIters.
 * Pair p owns rows [offsets[p], offsets[p+1]) of pts0/pts1 ([N][2] f64
 * pixels); cam [n_pairs][4] = fx, fy, cx, cy.  work [N][4] f64 scratch.
 * Out: E [n_pairs][10][9] (row-major; model 0 is the RANSAC result, all
 * models only when a pair has exactly 5 points), n_models (0 = no model,
 * cv2 returns None), mask [N] u8 0/1, n_inliers, iters (hypotheses drawn).
 * All pointers are device memory.                                            */
int sfmhip_find_essential(const double* pts0, const double* pts1, const int64_t* offsets,
                          int n_pairs, const double* cam, double prob, double threshold,
                          int max_iters, double* work, double* E, int32_t* n_models,
                          uint8_t* mask, int32_t* n_inliers, int32_t* iters, void* stream);

/* cv2.recoverPose(E, pts0, pts1, K) at matching.py:139, sfm.py:117,119
 * (distanceThresh = 50): decomposeEssentialMat + DLT cheirality of the 4
 * candidate poses.  E for pair p at E + p*e_stride (e_stride >= 9, 90 for
 * sfmhip_find_essential's output); mask_in [N] u8 or NULL (rows with 0 are
 * excluded, == recoverPose on the compacted points).  Out: R [n_pairs][9],
 * t [n_pairs][3], mask_out [N] u8 0/255, n_good [n_pairs].                   */
int sfmhip_recover_pose(const double* E, int64_t e_stride, const double* pts0, const double* pts1,
                        const int64_t* offsets, int n_pairs, const double* cam,
                        const uint8_t* mask_in, double distance_thresh, double* R, double* t,
                        uint8_t* mask_out, int32_t* n_good, void* stream);

/* cv2.findHomography(src, dst, cv2.RANSAC, ransacReprojThreshold=3, maxIters=2000,
 * confidence=0.995), batched over image pairs in sfmhip_find_essential's packed
 * layout (pixels; no camera): cv::RNG(-1) 4-point samples, checkSubset (no three
 * points collinear in either image, every triple keeps its orientation; a
 * rejected sample is one iteration without a model), Hartley-normalised DLT,
 * forward transfer error (float) <= threshold^2, a model replaces the best iff
 * count > max(best, 3), RANSACUpdateNumIters; the final H is the DLT over the
 * winning model's inliers (no Levenberg-Marquardt polish).
 * Out: H [n_pairs][9] (row-major, H[8] = 1; zeros where ok = 0), ok, mask [N]
 * u8 0/1 (the winning sample model's), n_inliers, iters (samples drawn).
 * All pointers are device memory.                                            */
int sfmhip_find_homography(const double* pts0, const double* pts1, const int64_t* offsets, int n_pairs,
                           double threshold, double confidence, int max_iters, double* H, int32_t* ok,
                           uint8_t* mask, int32_t* n_inliers, int32_t* iters, void* stream);

/* Parallax and image coverage of the correspondences that mask [N] u8 selects,
 * per pair (R [n_pairs][9] the relative rotation, cam [n_pairs][4] = fx, fy,
 * cx, cy; both images width x height pixels).  Out: cosang [N] f64, the cosine
 * of the angle between the rays K^-1 x0 and R^T K^-1 x1 (2.0 on unselected
 * rows); cover [n_pairs][2] u64, bit 8 floor(8y/height) + floor(8x/width) set
 * for every selected point inside [0, width) x [0, height) of image 0 / 1;
 * n_sel [n_pairs], the selected rows; median [n_pairs] f32, the lower median of
 * the pair's selected cosines rounded to float, by sfmhip_segmented_select
 * (2.0 when none is selected, NaN for an empty pair).  work [N] f32 and
 * rank_work [n_pairs] int64 are scratch.  All pointers are device memory.     */
int sfmhip_pair_stats(const double* pts0, const double* pts1, const int64_t* offsets, int n_pairs,
                      int64_t n_points, const uint8_t* mask, const double* R, const double* cam,
                      double width, double height, double* cosang, float* work, int64_t* rank_work,
                      uint64_t* cover, int32_t* n_sel, float* median, void* stream);

/* cv2.solvePnPRansac(X, pts1, K, zeros(5,1), cv2.SOLVEPNP_ITERATIVE) at
 * sfm.py:116 (iterationsCount 100, reprojectionError 8, confidence 0.99):
 * points converted to float, cv::RNG(-1) 5-point samples solved by EPnP,
 * float squared reprojection error <= reprojectionError^2, the RANSAC pose
 * refined on its inliers by CvLevMarq (20 iterations).  Problem p owns rows
 * [offsets[p], offsets[p+1]) of obj ([N][3] f64) / img ([N][2] f64 pixels);
 * cam [n][4] = fx, fy, cx, cy; work [N][5] f32 scratch.  Out: rvec/tvec
 * [n][3], inlier_mask [N] u8 (RANSAC inliers), n_inliers, iters, ok.
 * n < 5 is reported as ok = 0 (OpenCV would use P3P at n == 4).           */
int sfmhip_pnp_ransac(const double* obj, const double* img, const int64_t* offsets, int n_problems,
                      const double* cam, int iterations, double reprojection_error, double confidence,
                      float* work, double* rvec, double* tvec, uint8_t* inlier_mask, int32_t* n_inliers,
                      int32_t* iters, int32_t* ok, void* stream);

/* ---- §8f row 4: one grid training step (plenoxel.py:100-111, sdf.py:427-438)
 * Fused render forward + mse_loss(gt, rgb) gradient + analytic backward +
 * trilinear scatter-add into grad_vm (voxel-major (D,H,W,32), accumulated;
 * zero it via sfmhip_adam_step's zero_grad).  S <= 256.  Out: rgb [B][3],
 * sqerr [B] = sum_ch (rgb - gt)^2 (loss = sum(sqerr) / (3B)); touched
 * [D*H*W] u8 (nullable): set to 1 for every voxel the scatter adds to.      */
int sfmhip_render_train(const float* grid_vm, int D, int H, int W, const float* bmin, const float* bmax,
                        int mask_mode, const float* rays_o, const float* rays_d, const float* z,
                        const float* gt, int64_t B, int S, float* rgb, float* sqerr, float* grad_vm,
                        uint8_t* touched, void* stream);

/* torch.optim.Adam single-tensor step (weight_decay 0, amsgrad off) over n
 * f32 parameters (n % 4 == 0), step = the step count after increment;
 * zero_grad != 0 also clears grad (optimizer.zero_grad).                     */
int sfmhip_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     double lr, double beta1, double beta2, double eps, int64_t step, int zero_grad,
                     void* stream);

/* The same Adam step when the gradient is known to be 0 outside flagged
 * runs: flags [ceil(n / 2^flag_shift)] u8, one per 2^flag_shift parameters
 * (the trainer: one per 32-channel voxel line, set by sfmhip_render_train's
 * `touched`); unflagged gradients are neither read nor re-zeroed, and with
 * zero_grad the flags are cleared too.  Results equal sfmhip_adam_step's.     */
int sfmhip_adam_step_flagged(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             double lr, double beta1, double beta2, double eps, int64_t step, int zero_grad,
                             uint8_t* flags, int flag_shift, void* stream);

/* (D,H,W,32) voxel-major -> (C,D,H,W) reference layout (trainer export).     */
int sfmhip_grid_from_voxel_major(const float* grid_vm, int C, int D, int H, int W, float* grid,
                                 void* stream);

/* ---- V3: GradientBasedSampler's effective samples (sdf.py:154-180, 251-256)
 * Slab ray/AABB test: t_near = max(max_a min(t0, t1), 0), t_far = min_a max(t0,
 * t1), valid = t_far > t_near (NaN rays invalid).  Bounds are HOST float[3]. */
int sfmhip_ray_aabb(const float* rays_o, const float* rays_d, int64_t B, const float* bmin,
                    const float* bmax, float* t_near, float* t_far, uint8_t* valid, void* stream);

/* Stratified uniform samples (sample_uniform, sdf.py:167-180): z = t_near (1-t)
 * + t_far t with t = linspace(0,1,S); perturb: lower + (upper-lower) t_rand.  */
int sfmhip_stratified_samples(const float* t_near, const float* t_far, const float* t_rand, int64_t B,
                              int S, int perturb, float* z, void* stream);

/* ---- multi-GPU: the match-graph collective ---------
 * Thin C-ABI over RCCL (resolved with dlopen at first use: the RCCL already
 * mapped into the process, else $SFMHIP_RCCL, else /opt/rocm/lib/librccl.so.1).
 * The reference has no distributed code; these serve the pair-sharded
 * exhaustive matcher: every rank matches its pairs, then ONE all-gather of the
 * fixed-size matches0 block over xGMI gives every rank the full graph.
 *   one process per GPU: sfmhip_comm_unique_id (one rank) -> broadcast the 128
 *     bytes -> sfmhip_comm_init_rank on every rank (current HIP device);
 *   one process, several GPUs: sfmhip_comm_init_all(ndev, devs, comms[ndev]),
 *     each rank's collective issued between sfmhip_comm_group_start/_end.
 * sfmhip_allgather: `count` elements of SFMHIP_DT_* per rank from `send`,
 * recv = nranks * count elements in rank order; asynchronous on `stream`.    */
int sfmhip_comm_unique_id(void* id /* 128 bytes, host */);
int sfmhip_comm_init_rank(int nranks, const void* id, int rank, void** comm);
int sfmhip_comm_init_all(int ndev, const int* devs /* NULL = 0..ndev-1 */, void** comms /* [ndev] */);
int sfmhip_comm_info(void* comm, int* nranks, int* rank, int* device);
int sfmhip_allgather(void* comm, const void* send, void* recv, size_t count, int dtype, void* stream);
int sfmhip_comm_group_start(void);
int sfmhip_comm_group_end(void);
int sfmhip_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* SFMHIP_H */
