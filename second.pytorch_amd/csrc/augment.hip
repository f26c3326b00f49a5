// Training augmentation on the device (include/second_hip.h, "Training augmentation"): what the reference's prep_pointcloud does to one
// frame's points and boxes between loading and voxelising (second/data/preprocess.py:250-286), for a whole batch, without a host read.
//   sec_points_in_boxes_f32  -- box_np_ops.points_in_rbbox / points_count_rbbox (second/core/box_np_ops.py:728-739)
//   sec_noise_per_box_f32    -- preprocess.noise_per_box + _select_transform (second/core/preprocess.py:244-273, 478-484)
//   sec_augment_points_f32   -- points_transform_, random_flip, global_rotation_v2, global_scaling_v2, global_translate_ on the points
//   sec_augment_boxes_f32    -- box3d_transform_ and the same global stages on the boxes, filter_gt_box_outside_range_by_center,
//                               _dict_select (compaction) and limit_period
//   sec_db_sample_select_f32 / sec_db_sample_merge_points_f32 -- DataBaseSamplerV2.sample_all (second/core/sample_ops.py:95-216,
//                               238-285) and the merge of second/data/preprocess.py:210-249, run in front of the stages above
// Every count (points per frame, boxes per frame, boxes kept or accepted) is read from / written to device memory, so the calls
// capture into a hipGraph.  All arithmetic is plain fp32 (the library builds with -ffp-contract=off and without packed fp32).
#include "common.hpp"

namespace sec {

constexpr int kAugMaxTry = 128;        // tries per box sec_noise_per_box_f32 accepts
constexpr int kAugMaxBoxes = 512;      // boxes per frame whose BEV corners sec_noise_per_box_f32 keeps in LDS
constexpr int kPibChunk = 256;         // boxes staged per pass of k_points_in_boxes
constexpr float kPi = 3.14159265358979323846f;

// corners_norm * dims @ rot_mat_T + centre with rot_mat_T = [[cos, -sin], [sin, cos]] (box_np_ops.py:429-448): the reference's
// rotation of a row vector, used for box corners, for the points of a moved box and for the global rotation alike.
__device__ __forceinline__ void rot_row(float x, float y, float c, float s, float &ox, float &oy) {
    ox = x * c + y * s;
    oy = y * c - x * s;
}

// ------------------------------------------------------------------------------------------------ points in boxes
// grid (x, batch): the blocks of row y walk frame y's points with a grid stride, its boxes pass through LDS kPibChunk at a time as
// (centre, half extents, cos, sin).  A point is inside when, rotated into the box frame, it is strictly within the half extents:
// the faces themselves are outside, as in _points_in_convex_polygon_3d_jit (second/core/geometry.py:202-230, `sign >= 0`).
__global__ __launch_bounds__(kBlock) void k_points_in_boxes(const float *__restrict__ points, int pitch,
                                                            const int *__restrict__ point_offsets, const float *__restrict__ boxes,
                                                            const int *__restrict__ box_offsets, const unsigned char *__restrict__ valid,
                                                            int *__restrict__ first_box, int *__restrict__ box_counts) {
    __shared__ float s_box[kPibChunk][8];
    __shared__ int s_ok[kPibChunk];
    __shared__ int s_cnt[kPibChunk];
    const int b = blockIdx.y;
    const int p0 = point_offsets[b], p1 = point_offsets[b + 1];
    const int g0 = box_offsets[b], g1 = box_offsets[b + 1];
    const int stride = gridDim.x * kBlock;
    const int first = p0 + blockIdx.x * kBlock;
    if (first >= p1) return;                              // (block-uniform: no barrier is skipped by part of a block)
    const int rounds = (p1 - first + stride - 1) / stride;
    for (int c0 = g0; c0 < g1 || c0 == g0; c0 += kPibChunk) {
        const int nb = min(kPibChunk, g1 - c0);
        __syncthreads();
        for (int j = threadIdx.x; j < nb; j += kBlock) {
            const float *bx = boxes + (size_t)(c0 + j) * 7;
            float sn, cs;
            sincosf(bx[6], &sn, &cs);
            s_box[j][0] = bx[0]; s_box[j][1] = bx[1]; s_box[j][2] = bx[2];
            s_box[j][3] = 0.5f * bx[3]; s_box[j][4] = 0.5f * bx[4]; s_box[j][5] = 0.5f * bx[5];
            s_box[j][6] = cs; s_box[j][7] = sn;
            s_ok[j] = valid ? (int)valid[c0 + j] : 1;
            s_cnt[j] = 0;
        }
        __syncthreads();
        for (int r = 0; r < rounds; ++r) {
            const int i = first + r * stride + threadIdx.x;
            if (i >= p1) continue;
            const float px = points[(size_t)i * pitch], py = points[(size_t)i * pitch + 1], pz = points[(size_t)i * pitch + 2];
            int hit = c0 == g0 ? -1 : first_box[i];
            for (int j = 0; j < nb; ++j) {
                const float dx = px - s_box[j][0], dy = py - s_box[j][1], dz = pz - s_box[j][2];
                const float lx = dx * s_box[j][6] - dy * s_box[j][7];       // the inverse of rot_row
                const float ly = dx * s_box[j][7] + dy * s_box[j][6];
                if (fabsf(lx) < s_box[j][3] && fabsf(ly) < s_box[j][4] && fabsf(dz) < s_box[j][5]) {
                    if (box_counts) atomicAdd(&s_cnt[j], 1);
                    if (hit < 0 && s_ok[j]) hit = c0 + j;
                }
            }
            first_box[i] = hit;
        }
        if (box_counts) {
            __syncthreads();
            for (int j = threadIdx.x; j < nb; j += kBlock)
                if (s_cnt[j]) atomicAdd(&box_counts[c0 + j], s_cnt[j]);   // integer: the total does not depend on arrival order
        }
    }
}

// ------------------------------------------------------------------------------------------------ per-object noise
// box_collision_test (second/core/preprocess.py:803-883) for one pair of BEV rectangles, corners a / b as [4][2], standup boxes
// sa / sb = (xmin, ymin, xmax, ymax).  The edge predicates are the four strict comparisons of the reference, term for term.  The
// containment branch follows the compiled (numba) meaning of `ret[i, j] is False`: a rectangle wholly inside the other collides.
__device__ __forceinline__ bool contains_all(const float *a, const float *q) {      // every corner of q strictly inside a
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float vx = a[2 * k1] - a[2 * k], vy = a[2 * k1 + 1] - a[2 * k + 1];    // -(a[k] - a[k+1]): clockwise
            float cross = vy * (a[2 * k] - q[2 * l]);
            cross -= vx * (a[2 * k + 1] - q[2 * l + 1]);
            if (cross >= 0.0f) return false;
        }
    return true;
}
__device__ __forceinline__ bool boxes_collide(const float *a, const float *sa, const float *b, const float *sb) {
    const float iw = fminf(sa[2], sb[2]) - fmaxf(sa[0], sb[0]);
    if (!(iw > 0.0f)) return false;
    const float ih = fminf(sa[3], sb[3]) - fmaxf(sa[1], sb[1]);
    if (!(ih > 0.0f)) return false;
    for (int k = 0; k < 4; ++k) {
        const float ax = a[2 * k], ay = a[2 * k + 1], bx = a[2 * ((k + 1) & 3)], by = a[2 * ((k + 1) & 3) + 1];
        for (int l = 0; l < 4; ++l) {
            const float cx = b[2 * l], cy = b[2 * l + 1], dx = b[2 * ((l + 1) & 3)], dy = b[2 * ((l + 1) & 3) + 1];
            const bool acd = (dy - ay) * (cx - ax) > (cy - ay) * (dx - ax);
            const bool bcd = (dy - by) * (cx - bx) > (cy - by) * (dx - bx);
            if (acd != bcd) {
                const bool abc = (cy - ay) * (bx - ax) > (by - ay) * (cx - ax);
                const bool abd = (dy - ay) * (bx - ax) > (by - ay) * (dx - ax);
                if (abc != abd) return true;
            }
        }
    }
    return contains_all(a, b) || contains_all(b, a);
}
__device__ __forceinline__ void standup_of(const float *c, float *s) {
    s[0] = fminf(fminf(c[0], c[2]), fminf(c[4], c[6]));
    s[1] = fminf(fminf(c[1], c[3]), fminf(c[5], c[7]));
    s[2] = fmaxf(fmaxf(c[0], c[2]), fmaxf(c[4], c[6]));
    s[3] = fmaxf(fmaxf(c[1], c[3]), fmaxf(c[5], c[7]));
}

// One workgroup per frame.  The frame's CURRENT corners live in LDS: a box that took a try is seen at its new place by the boxes after
// it, an invalid box never moves but blocks (preprocess.py:257-272).  Only the walk over the boxes is sequential: for box i the
// workgroup builds every try's rectangle, then tests (try, other box) pairs a round of tries at a time -- as many tries as fill the
// 256 lanes -- and stops at the first round that holds a collision-free try; the lowest such try wins.
__global__ __launch_bounds__(kBlock) void k_noise_per_box(const float *__restrict__ boxes, const int *__restrict__ box_offsets,
                                                          int n_boxes, int batch, const unsigned char *__restrict__ valid,
                                                          const float *__restrict__ loc_noises, const float *__restrict__ rot_noises,
                                                          int num_try, int max_boxes, int *__restrict__ selected,
                                                          float *__restrict__ loc_transform, float *__restrict__ rot_transform) {
    __shared__ float s_cur[kAugMaxBoxes][8];      // current corners
    __shared__ float s_std[kAugMaxBoxes][4];      // and their standup boxes
    __shared__ float s_try[kAugMaxTry][8];
    __shared__ float s_tstd[kAugMaxTry][4];
    __shared__ int s_hit[kAugMaxTry];
    __shared__ int s_best;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = box_offsets[b], g1 = box_offsets[b + 1];
    const int n = g1 - g0;
    if (b == 0)                                   // capacity rows behind the last frame: no transform
        for (int g = box_offsets[batch] + tid; g < n_boxes; g += kBlock) {
            selected[g] = -1; rot_transform[g] = 0.0f;
            loc_transform[3 * g] = 0.0f; loc_transform[3 * g + 1] = 0.0f; loc_transform[3 * g + 2] = 0.0f;
        }
    for (int j = tid; j < n; j += kBlock) {
        const int g = g0 + j;
        selected[g] = -1; rot_transform[g] = 0.0f;
        loc_transform[3 * g] = 0.0f; loc_transform[3 * g + 1] = 0.0f; loc_transform[3 * g + 2] = 0.0f;
    }
    if (n <= 0 || n > max_boxes) return;          // more boxes than the LDS table holds: the frame keeps its boxes (documented)
    for (int j = tid; j < n; j += kBlock) {
        const float *bx = boxes + (size_t)(g0 + j) * 7;
        float sn, cs;
        sincosf(bx[6], &sn, &cs);
        const float hw = 0.5f * bx[3], hl = 0.5f * bx[4];
        const float lx[4] = {-hw, -hw, hw, hw}, ly[4] = {-hl, hl, hl, -hl};       // clockwise from the minimum corner
        for (int k = 0; k < 4; ++k) {
            float x, y;
            rot_row(lx[k], ly[k], cs, sn, x, y);
            s_cur[j][2 * k] = x + bx[0]; s_cur[j][2 * k + 1] = y + bx[1];
        }
        standup_of(s_cur[j], s_std[j]);
    }
    __syncthreads();
    const int per_round = max(1, min(num_try, kBlock / n));       // tries tested per round
    for (int i = 0; i < n; ++i) {
        const int g = g0 + i;
        if (valid && !valid[g]) continue;                          // (uniform over the workgroup)
        const float cx = boxes[(size_t)g * 7], cy = boxes[(size_t)g * 7 + 1];
        if (tid < num_try) {
            float sn, cs;
            sincosf(rot_noises[(size_t)g * num_try + tid], &sn, &cs);
            const float *ln = loc_noises + ((size_t)g * num_try + tid) * 3;
            for (int k = 0; k < 4; ++k) {
                float x, y;
                rot_row(s_cur[i][2 * k] - cx, s_cur[i][2 * k + 1] - cy, cs, sn, x, y);
                s_try[tid][2 * k] = x + (cx + ln[0]); s_try[tid][2 * k + 1] = y + (cy + ln[1]);
            }
            standup_of(s_try[tid], s_tstd[tid]);
            s_hit[tid] = 0;
        }
        if (tid == 0) s_best = num_try;
        __syncthreads();
        for (int t0 = 0; t0 < num_try; t0 += per_round) {
            const int nt = min(per_round, num_try - t0);
            for (int p = tid; p < nt * n; p += kBlock) {
                const int t = t0 + p / n, j = p % n;
                if (j != i && boxes_collide(s_try[t], s_tstd[t], s_cur[j], s_std[j])) s_hit[t] = 1;
            }
            __syncthreads();
            if (tid < nt && !s_hit[t0 + tid]) atomicMin(&s_best, t0 + tid);
            __syncthreads();
            if (s_best < num_try) break;                           // (uniform: every thread reads the same word after the barrier)
        }
        const int best = s_best;
        if (best < num_try) {
            if (tid < 8) s_cur[i][tid] = s_try[best][tid];
            if (tid >= 8 && tid < 12) s_std[i][tid - 8] = s_tstd[best][tid - 8];
            if (tid == 12) {
                const float *ln = loc_noises + ((size_t)g * num_try + best) * 3;
                selected[g] = best;
                loc_transform[3 * g] = ln[0]; loc_transform[3 * g + 1] = ln[1]; loc_transform[3 * g + 2] = ln[2];
                rot_transform[g] = rot_noises[(size_t)g * num_try + best];
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ points, one pass
// frame_params[b] = (flip_x, flip_y, angle, scale, tx, ty, tz, 0).  Per point: the transform of its first valid containing box about
// that box's ORIGINAL centre (points_transform_, preprocess.py:450-466), then the frame's flips, rotation, scaling and translation in
// prep_pointcloud's order (second/data/preprocess.py:273-279).
__global__ __launch_bounds__(kBlock) void k_augment_points(float *__restrict__ points, int pitch, const int *__restrict__ point_offsets,
                                                           const int *__restrict__ first_box, const float *__restrict__ boxes,
                                                           const unsigned char *__restrict__ valid,
                                                           const float *__restrict__ loc_transform,
                                                           const float *__restrict__ rot_transform,
                                                           const float *__restrict__ frame_params) {
    const int b = blockIdx.y;
    const int p1 = point_offsets[b + 1];
    const float *fp = frame_params + (size_t)b * 8;
    const bool flip_x = fp[0] != 0.0f, flip_y = fp[1] != 0.0f;
    const float scale = fp[3], tx = fp[4], ty = fp[5], tz = fp[6];
    float gs, gc;
    sincosf(fp[2], &gs, &gc);
    const int stride = gridDim.x * kBlock;
    for (int i = point_offsets[b] + blockIdx.x * kBlock + threadIdx.x; i < p1; i += stride) {
        float *p = points + (size_t)i * pitch;
        float x = p[0], y = p[1], z = p[2];
        const int g = first_box ? first_box[i] : -1;
        if (g >= 0 && (!valid || valid[g])) {
            const float *bx = boxes + (size_t)g * 7;
            float sn, cs, rx, ry;
            sincosf(rot_transform[g], &sn, &cs);
            rot_row(x - bx[0], y - bx[1], cs, sn, rx, ry);
            x = rx + bx[0] + loc_transform[3 * g];
            y = ry + bx[1] + loc_transform[3 * g + 1];
            z = (z - bx[2]) + bx[2] + loc_transform[3 * g + 2];
        }
        if (flip_y) y = -y;
        if (flip_x) x = -x;
        float rx, ry;
        rot_row(x, y, gc, gs, rx, ry);
        p[0] = rx * scale + tx; p[1] = ry * scale + ty; p[2] = z * scale + tz;
    }
}

// ------------------------------------------------------------------------------------------------ boxes: transform, filter, compact
// One workgroup walks the frames in order, 256 boxes at a time; a block scan of the keep flags places the survivors of a frame
// behind those of the frames before it, in their original order.  Rows behind the last survivor are zeroed.
// VELO: rows of 9 values, columns 7 and 8 a velocity (vx, vy) that the flips, the rotation and the scaling transform as the reference
// does for shape[1] == 9 (preprocess.py:749-799); translation, per-object noise and the yaw wrap leave it alone.
template <bool VELO>
__device__ __forceinline__ void augment_boxes_body(const float *__restrict__ boxes, const int *__restrict__ box_offsets, int n_boxes,
                                                   int batch, const unsigned char *__restrict__ valid,
                                                   const int *__restrict__ classes, const float *__restrict__ importance,
                                                   const float *__restrict__ loc_transform,
                                                   const float *__restrict__ rot_transform,
                                                   const float *__restrict__ frame_params, float xmin, float ymin, float xmax,
                                                   float ymax, float *__restrict__ out_boxes, int *__restrict__ out_classes,
                                                   float *__restrict__ out_importance, int *__restrict__ out_offsets) {
    constexpr int ND = VELO ? 9 : 7;
    __shared__ int s_scan[8];
    const int tid = threadIdx.x;
    int base = 0;
    if (tid == 0) out_offsets[0] = 0;
    for (int b = 0; b < batch; ++b) {
        const int g0 = box_offsets[b], g1 = box_offsets[b + 1];
        const float *fp = frame_params + (size_t)b * 8;
        const bool flip_x = fp[0] != 0.0f, flip_y = fp[1] != 0.0f;
        const float angle = fp[2], scale = fp[3];
        float gs, gc;
        sincosf(angle, &gs, &gc);
        for (int c0 = g0; c0 < g1; c0 += kBlock) {
            const int g = c0 + tid;
            float v[7] = {0, 0, 0, 0, 0, 0, 0};
            float vx = 0.0f, vy = 0.0f;
            int keep = 0;
            if (g < g1) {
                for (int k = 0; k < 7; ++k) v[k] = boxes[(size_t)g * ND + k];
                if (VELO) { vx = boxes[(size_t)g * ND + 7]; vy = boxes[(size_t)g * ND + 8]; }
                const bool ok = !valid || valid[g];
                if (ok && loc_transform) {                          // box3d_transform_ (preprocess.py:469-475)
                    v[0] += loc_transform[3 * g]; v[1] += loc_transform[3 * g + 1]; v[2] += loc_transform[3 * g + 2];
                    v[6] += rot_transform[g];
                }
                if (flip_y) { v[1] = -v[1]; v[6] = -v[6] + kPi; }   // random_flip (preprocess.py:749-769)
                if (flip_x) { v[0] = -v[0]; v[6] = -v[6]; }
                float rx, ry;
                rot_row(v[0], v[1], gc, gs, rx, ry);                // global_rotation_v2 (preprocess.py:781-799)
                v[6] += angle;
                if (VELO) {
                    if (flip_y) vy = -vy;
                    if (flip_x) vx = -vx;
                    float wx, wy;
                    rot_row(vx, vy, gc, gs, wx, wy);                // gt_boxes[:, 7:9] @ [[c, -s], [s, c]]
                    vx = wx * scale; vy = wy * scale;
                }
                v[0] = rx * scale + fp[4]; v[1] = ry * scale + fp[5]; v[2] = v[2] * scale + fp[6];       // global_scaling_v2, global_translate_
                v[3] *= scale; v[4] *= scale; v[5] *= scale;
                keep = ok && v[0] > xmin && v[0] < xmax && v[1] > ymin && v[1] < ymax;   // filter_gt_box_outside_range_by_center: the edge is outside
                v[6] = v[6] - floorf(v[6] / (2.0f * kPi) + 0.5f) * (2.0f * kPi);         // limit_period(yaw, 0.5, 2 pi)
            }
            int total;
            const int pos = base + block_exclusive_scan(keep, s_scan, &total);
            if (keep) {
                for (int k = 0; k < 7; ++k) out_boxes[(size_t)pos * ND + k] = v[k];
                if (VELO) { out_boxes[(size_t)pos * ND + 7] = vx; out_boxes[(size_t)pos * ND + 8] = vy; }
                if (out_classes) out_classes[pos] = classes ? classes[g] : 1;
                if (out_importance) out_importance[pos] = importance ? importance[g] : 1.0f;
            }
            base += total;
        }
        if (tid == 0) out_offsets[b + 1] = base;
    }
    for (int g = base + tid; g < n_boxes; g += kBlock) {
        for (int k = 0; k < ND; ++k) out_boxes[(size_t)g * ND + k] = 0.0f;
        if (out_classes) out_classes[g] = 0;
        if (out_importance) out_importance[g] = 0.0f;
    }
}
__global__ __launch_bounds__(kBlock) void k_augment_boxes(const float *__restrict__ boxes, const int *__restrict__ box_offsets, int n_boxes,
                                                          int batch, const unsigned char *__restrict__ valid,
                                                          const int *__restrict__ classes, const float *__restrict__ importance,
                                                          const float *__restrict__ loc_transform,
                                                          const float *__restrict__ rot_transform,
                                                          const float *__restrict__ frame_params, float xmin, float ymin, float xmax,
                                                          float ymax, float *__restrict__ out_boxes, int *__restrict__ out_classes,
                                                          float *__restrict__ out_importance, int *__restrict__ out_offsets) {
    augment_boxes_body<false>(boxes, box_offsets, n_boxes, batch, valid, classes, importance, loc_transform, rot_transform, frame_params, xmin,
                              ymin, xmax, ymax, out_boxes, out_classes, out_importance, out_offsets);
}
__global__ __launch_bounds__(kBlock) void k_augment_boxes_velo(const float *__restrict__ boxes, const int *__restrict__ box_offsets, int n_boxes,
                                                               int batch, const unsigned char *__restrict__ valid,
                                                               const int *__restrict__ classes, const float *__restrict__ importance,
                                                               const float *__restrict__ loc_transform,
                                                               const float *__restrict__ rot_transform,
                                                               const float *__restrict__ frame_params, float xmin, float ymin, float xmax,
                                                               float ymax, float *__restrict__ out_boxes, int *__restrict__ out_classes,
                                                               float *__restrict__ out_importance, int *__restrict__ out_offsets) {
    augment_boxes_body<true>(boxes, box_offsets, n_boxes, batch, valid, classes, importance, loc_transform, rot_transform, frame_params, xmin,
                             ymin, xmax, ymax, out_boxes, out_classes, out_importance, out_offsets);
}

// blocks per frame for the two point kernels: the frames' sizes are device data, so the grid is sized for frames of the mean size
// and a grid stride covers the rest
static int point_blocks(int n_points, int batch) {
    const int b = div_up(2LL * div_up(n_points > 0 ? n_points : 1, batch), kBlock);
    return b < 1 ? 1 : (b > 256 ? 256 : b);
}

// ------------------------------------------------------------------------------------------------ database sampling: acceptance
// DataBaseSamplerV2.sample_all / sample_class_v2 (second/core/sample_ops.py:95-160, 238-285) for single-class groups without the
// sampler's rotation.  One workgroup per frame.  s_cur holds the BEV corners of `avoid`: the frame's gt boxes, then what earlier
// groups accepted.  Per group the workgroup builds the corners of the candidates in use, tests every (candidate, avoid box) and
// (candidate, candidate) pair in parallel -- s_hit[i]: candidate i meets an avoid box; s_cc[i]: a 64-bit row of the candidate x
// candidate matrix -- and thread 0 walks the candidates as the reference walks its matrix: candidate i is rejected if its row still
// has an entry, and only a rejected candidate's column is cleared, when the walk reaches it.  So later candidates block whether or
// not they end up accepted; earlier ones only if they were accepted.
constexpr int kDbMaxK = 64;            // candidates per frame and group
constexpr int kDbMaxGroups = 16;

__device__ __forceinline__ void bev_corners_of(const float *bx, float *c, float *s) {
    float sn, cs;
    sincosf(bx[6], &sn, &cs);
    const float hw = 0.5f * bx[3], hl = 0.5f * bx[4];
    const float lx[4] = {-hw, -hw, hw, hw}, ly[4] = {-hl, hl, hl, -hl};           // clockwise from the minimum corner
    for (int k = 0; k < 4; ++k) {
        float x, y;
        rot_row(lx[k], ly[k], cs, sn, x, y);
        c[2 * k] = x + bx[0]; c[2 * k + 1] = y + bx[1];
    }
    standup_of(c, s);
}

__global__ __launch_bounds__(kBlock) void k_db_select(const float *__restrict__ gt_boxes, const int *__restrict__ gt_offsets, int n_gt,
                                                      const int *__restrict__ gt_classes, const float *__restrict__ db_boxes, int n_db,
                                                      const int *__restrict__ candidates, int groups, int k,
                                                      const int *__restrict__ class_of_group, const int *__restrict__ num_table,
                                                      int table_len, int *__restrict__ accepted, int *__restrict__ accepted_count,
                                                      int *__restrict__ accepted_per_group) {
    __shared__ float s_cur[kAugMaxBoxes][8];
    __shared__ float s_std[kAugMaxBoxes][4];
    __shared__ float s_cand[kDbMaxK][8];
    __shared__ float s_cstd[kDbMaxK][4];
    __shared__ int s_row[kDbMaxK];
    __shared__ int s_hit[kDbMaxK];
    __shared__ unsigned s_cc[kDbMaxK][2];
    __shared__ int s_take[kDbMaxK];
    __shared__ int s_cnt[kDbMaxGroups];
    __shared__ int s_m[kDbMaxGroups];
    __shared__ int s_scan[8];
    __shared__ int s_took;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = max(gt_offsets[b], 0), g1 = min(gt_offsets[b + 1], n_gt);
    const int n = max(g1 - g0, 0);
    int *acc = accepted + (size_t)b * groups * k;
    for (int j = tid; j < groups * k; j += kBlock) acc[j] = -1;
    if (tid < groups) { s_cnt[tid] = 0; accepted_per_group[b * groups + tid] = 0; }
    __syncthreads();
    for (int j = tid; j < n; j += kBlock) {                       // gt boxes per sample class: every box counts, masked or not
        const int cls = gt_classes ? gt_classes[g0 + j] : 1;
        for (int c = 0; c < groups; ++c)
            if (cls > 0 && cls == class_of_group[c]) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    if (tid < groups) {                                           // candidates in use: min(sampled_num, candidates present)
        int present = 0;
        for (int q = 0; q < k; ++q) {
            const int v = candidates[((size_t)b * groups + tid) * k + q];
            present += v >= 0 && v < n_db;
        }
        const int want = s_cnt[tid] < table_len ? num_table[tid * table_len + s_cnt[tid]] : 0;
        s_m[tid] = min(max(want, 0), present);
    }
    __syncthreads();
    int total = n;
    for (int c = 0; c < groups; ++c) total += s_m[c];
    if (total > kAugMaxBoxes) {                                   // more than the LDS table holds: the frame keeps its gt (documented)
        if (tid == 0) accepted_count[b] = 0;
        return;
    }
    for (int j = tid; j < n; j += kBlock) bev_corners_of(gt_boxes + (size_t)(g0 + j) * 7, s_cur[j], s_std[j]);
    int avoid = n, n_acc = 0;
    for (int c = 0; c < groups; ++c) {
        const int m = s_m[c];
        if (m == 0) continue;                                     // (uniform over the workgroup)
        const int v = tid < k ? candidates[((size_t)b * groups + c) * k + tid] : -1;
        const int ok = v >= 0 && v < n_db;
        int present;
        const int pos = block_exclusive_scan(ok, s_scan, &present);
        if (ok && pos < m) {
            s_row[pos] = v;
            bev_corners_of(db_boxes + (size_t)v * 7, s_cand[pos], s_cstd[pos]);
            s_hit[pos] = 0; s_cc[pos][0] = 0u; s_cc[pos][1] = 0u;
        }
        __syncthreads();                                          // (also orders s_cur: the gt corners, the rows the last group added)
        const int cols = avoid + m;
        for (int p = tid; p < m * cols; p += kBlock) {
            const int i = p / cols, j = p % cols, q = j - avoid;          // q >= 0: the other box is candidate q
            if (q == i) continue;
            const float *oc = q >= 0 ? s_cand[q] : s_cur[j], *os = q >= 0 ? s_cstd[q] : s_std[j];
            if (!boxes_collide(s_cand[i], s_cstd[i], oc, os)) continue;
            if (q >= 0) atomicOr(&s_cc[i][q >> 5], 1u << (q & 31));
            else s_hit[i] = 1;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rej0 = 0u, rej1 = 0u;
            int took = 0;
            for (int i = 0; i < m; ++i) {
                if (s_hit[i] || (s_cc[i][0] & ~rej0) || (s_cc[i][1] & ~rej1)) {
                    if (i < 32) rej0 |= 1u << i; else rej1 |= 1u << (i - 32);
                    s_take[i] = -1;
                } else {
                    s_take[i] = took++;
                }
            }
            s_took = took;
            accepted_per_group[b * groups + c] = took;
        }
        __syncthreads();
        if (tid < m && s_take[tid] >= 0) {
            const int d = avoid + s_take[tid];
            for (int e = 0; e < 8; ++e) s_cur[d][e] = s_cand[tid][e];
            for (int e = 0; e < 4; ++e) s_std[d][e] = s_cstd[tid][e];
            acc[n_acc + s_take[tid]] = s_row[tid];
        }
        const int took = s_took;
        avoid += took; n_acc += took;
        __syncthreads();
    }
    if (tid == 0) accepted_count[b] = n_acc;
}

// The merge of second/data/preprocess.py:229-237 on the boxes: per frame the gt rows, unchanged and in order, then the accepted
// boxes.  A launch of its own: frame b's place depends on what the frames before it accepted.
__global__ __launch_bounds__(kBlock) void k_db_merge_boxes(const float *__restrict__ gt_boxes, const int *__restrict__ gt_offsets, int n_gt,
                                                           int batch, const int *__restrict__ gt_classes,
                                                           const unsigned char *__restrict__ gt_valid,
                                                           const float *__restrict__ gt_importance, const float *__restrict__ db_boxes,
                                                           int n_db, int groups, int k, const int *__restrict__ class_of_group,
                                                           float sample_importance, const int *__restrict__ accepted,
                                                           const int *__restrict__ accepted_count,
                                                           const int *__restrict__ accepted_per_group, float *__restrict__ out_boxes,
                                                           int capacity, int *__restrict__ out_classes, unsigned char *__restrict__ out_valid,
                                                           float *__restrict__ out_importance, unsigned char *__restrict__ out_sampled,
                                                           int *__restrict__ out_offsets) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int first = max(gt_offsets[0], 0);
    const int g0 = max(gt_offsets[b], 0), g1 = min(gt_offsets[b + 1], n_gt);
    const int n = max(g1 - g0, 0);
    int before = 0, all = 0;
    for (int f = 0; f < batch; ++f) {
        const int a = min(max(accepted_count[f], 0), groups * k);
        if (f < b) before += a;
        all += a;
    }
    const int cnt = min(max(accepted_count[b], 0), groups * k);
    const int base = max(g0 - first, 0) + before;
    const int end = max(min(gt_offsets[batch], n_gt) - first, 0) + all;
    if (tid == 0) {
        out_offsets[b] = min(base, capacity);
        if (b == batch - 1) out_offsets[batch] = min(end, capacity);
    }
    for (int j = tid; j < n + cnt; j += kBlock) {
        const int o = base + j;
        if (o >= capacity) break;
        const bool gt = j < n;
        int row = gt ? g0 + j : accepted[(size_t)b * groups * k + (j - n)];
        const float *src = gt ? gt_boxes : db_boxes;
        if (!gt && (row < 0 || row >= n_db)) row = 0;                               // (k_db_select writes rows of the database only)
        for (int e = 0; e < 7; ++e) out_boxes[(size_t)o * 7 + e] = src[(size_t)row * 7 + e];
        int cls = 0;
        if (gt) {
            cls = gt_classes ? gt_classes[row] : 1;
        } else {
            int a = j - n;
            for (int c = 0; c < groups; ++c) {
                const int t = accepted_per_group[b * groups + c];
                if (a < t) { cls = class_of_group[c]; break; }
                a -= t;
            }
        }
        if (out_classes) out_classes[o] = cls;
        if (out_valid) out_valid[o] = gt ? (gt_valid ? gt_valid[row] : 1) : 1;
        if (out_importance) out_importance[o] = gt ? (gt_importance ? gt_importance[row] : 1.0f) : sample_importance;
        if (out_sampled) out_sampled[o] = gt ? 0 : 1;
    }
    for (int o = max(end, 0) + b * kBlock + tid; o < capacity; o += batch * kBlock) {
        for (int e = 0; e < 7; ++e) out_boxes[(size_t)o * 7 + e] = 0.0f;
        if (out_classes) out_classes[o] = 0;
        if (out_valid) out_valid[o] = 0;
        if (out_importance) out_importance[o] = 0.0f;
        if (out_sampled) out_sampled[o] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ database sampling: the points
// points = concatenate([sampled_points, points[~removed]]) per frame (second/data/preprocess.py:244-249), stable, in three launches:
// keep counts per 256 rows of the flat point array; one workgroup that scans them, sizes every frame (accepted objects' points +
// survivors) and places frames and objects; the scatter.  Workspace (ints): [blocks] keep prefix, [batch + 1] frame start,
// [batch] keep prefix at the frame's first point, [batch] sampled points of the frame, [batch * slots] start of every accepted
// object inside its frame.
struct DbMergeWs {
    int *blk, *start, *kp0, *sampled, *obj;
};
static size_t db_merge_ws_ints(int n_points, int batch, int slots) {
    return (size_t)div_up(n_points > 0 ? n_points : 1, kBlock) + 3 * (size_t)batch + 1 + (size_t)batch * slots;
}
static DbMergeWs db_merge_ws(void *ws, int n_points, int batch, int slots) {
    DbMergeWs w;
    w.blk = (int *)ws;
    w.start = w.blk + div_up(n_points > 0 ? n_points : 1, kBlock);
    w.kp0 = w.start + batch + 1;
    w.sampled = w.kp0 + batch;
    w.obj = w.sampled + batch;
    return w;
}

__device__ __forceinline__ int dbm_keep(int i, int lo, int hi, const int *__restrict__ first_box) {
    return i >= lo && i < hi && !(first_box && first_box[i] >= 0);
}

__global__ __launch_bounds__(kBlock) void k_dbm_count(const int *__restrict__ point_offsets, int n_points, int batch,
                                                      const int *__restrict__ first_box, int *__restrict__ blk) {
    __shared__ int s_scan[8];
    const int lo = max(point_offsets[0], 0), hi = min(point_offsets[batch], n_points);
    int total;
    block_exclusive_scan(dbm_keep(blockIdx.x * kBlock + threadIdx.x, lo, hi, first_box), s_scan, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_dbm_scan(const int *__restrict__ point_offsets, int n_points, int batch,
                                                     const int *__restrict__ first_box, const int *__restrict__ pool_offsets, int n_db,
                                                     const int *__restrict__ accepted, const int *__restrict__ accepted_count, int slots,
                                                     int n_blocks, DbMergeWs w, int capacity, int *__restrict__ out_offsets,
                                                     int *__restrict__ overflow) {
    __shared__ int s_scan[8];
    const int tid = threadIdx.x;
    const int lo = max(point_offsets[0], 0), hi = min(point_offsets[batch], n_points);
    int kept_all = 0;
    for (int c0 = 0; c0 < n_blocks; c0 += kBlock) {
        const int t = c0 + tid;
        int total;
        const int ex = block_exclusive_scan(t < n_blocks ? w.blk[t] : 0, s_scan, &total);
        if (t < n_blocks) w.blk[t] = kept_all + ex;
        kept_all += total;
    }
    __syncthreads();
    int start = 0;
    for (int b = 0; b < batch; ++b) {
        const int p0 = min(max(point_offsets[b], lo), hi), p1 = min(max(point_offsets[b + 1], p0), hi);
        int kp[2];
        for (int s = 0; s < 2; ++s) {                             // survivors in front of p0 / p1: whole blocks + the rows of a part block
            const int p = s ? p1 : p0;
            const int t = p / kBlock, r = p % kBlock;
            int part;
            block_exclusive_scan(tid < r ? dbm_keep(t * kBlock + tid, lo, hi, first_box) : 0, s_scan, &part);
            kp[s] = (t < n_blocks ? w.blk[t] : kept_all) + part;
        }
        const int cnt = min(max(accepted_count[b], 0), slots);
        int sampled = 0;
        for (int a0 = 0; a0 < cnt; a0 += kBlock) {
            const int a = a0 + tid;
            int len = 0;
            if (a < cnt) {
                const int r = accepted[(size_t)b * slots + a];
                if (r >= 0 && r < n_db) len = max(pool_offsets[r + 1] - pool_offsets[r], 0);
            }
            int total;
            const int ex = block_exclusive_scan(len, s_scan, &total);
            if (a < cnt) w.obj[(size_t)b * slots + a] = sampled + ex;
            sampled += total;
        }
        if (tid == 0) {
            w.start[b] = start; w.kp0[b] = kp[0]; w.sampled[b] = sampled;
            out_offsets[b] = min(start, capacity);
        }
        start += sampled + (kp[1] - kp[0]);
    }
    if (tid == 0) {
        w.start[batch] = start;
        out_offsets[batch] = min(start, capacity);
        *overflow = start > capacity ? 1 : 0;
    }
}

// blocks [0, n_blocks): the survivors of 256 rows; blocks behind them: one accepted object each (frame, slot)
__global__ __launch_bounds__(kBlock) void k_dbm_scatter(const float *__restrict__ points, int pitch, const int *__restrict__ point_offsets,
                                                        int n_points, int batch, const int *__restrict__ first_box,
                                                        const float *__restrict__ pool_points, const int *__restrict__ pool_offsets,
                                                        const float *__restrict__ db_boxes, int n_db, const int *__restrict__ accepted,
                                                        const int *__restrict__ accepted_count, int slots, int n_blocks, DbMergeWs w,
                                                        float *__restrict__ out_points, int capacity) {
    __shared__ int s_scan[8];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_blocks) {
        const int lo = max(point_offsets[0], 0), hi = min(point_offsets[batch], n_points);
        const int i = blockIdx.x * kBlock + tid;
        const int keep = dbm_keep(i, lo, hi, first_box);
        int total;
        const int ex = block_exclusive_scan(keep, s_scan, &total);
        if (!keep) return;
        int f0 = 0, f1 = batch - 1;                               // the frame that owns row i
        while (f0 < f1) {
            const int mid = (f0 + f1) >> 1;
            if (point_offsets[mid + 1] <= i) f0 = mid + 1; else f1 = mid;
        }
        const int d = w.start[f0] + w.sampled[f0] + (w.blk[blockIdx.x] + ex - w.kp0[f0]);
        if (d < 0 || d >= capacity) return;
        for (int e = 0; e < pitch; ++e) out_points[(size_t)d * pitch + e] = points[(size_t)i * pitch + e];
        return;
    }
    const int q = blockIdx.x - n_blocks;
    const int b = q / slots, a = q % slots;
    if (a >= min(accepted_count[b], slots)) return;
    const int r = accepted[q];
    if (r < 0 || r >= n_db) return;
    const int s0 = pool_offsets[r], len = pool_offsets[r + 1] - s0;
    const int d0 = w.start[b] + w.obj[q];
    const float cx = db_boxes[(size_t)r * 7], cy = db_boxes[(size_t)r * 7 + 1], cz = db_boxes[(size_t)r * 7 + 2];
    for (int j = tid; j < len; j += kBlock) {
        const int d = d0 + j;
        if (d < 0 || d >= capacity) break;
        const float *src = pool_points + (size_t)(s0 + j) * pitch;
        float *dst = out_points + (size_t)d * pitch;
        dst[0] = src[0] + cx; dst[1] = src[1] + cy; dst[2] = src[2] + cz;     // s_points[:, :3] += box3d_lidar[:3]: one fp32 add
        for (int e = 3; e < pitch; ++e) dst[e] = src[e];
    }
}

}  // namespace sec

using namespace sec;

SEC_API int sec_points_in_boxes_f32(const float *points, int point_pitch, const int *point_offsets, int n_points, const float *boxes,
                                    const int *box_offsets, int n_boxes, int batch, const unsigned char *valid, int *first_box,
                                    int *box_counts, void *stream) {
    if (batch <= 0 || n_points < 0 || n_boxes < 0 || !point_offsets || !box_offsets || !first_box || (n_points > 0 && !points) ||
        (n_boxes > 0 && !boxes))
        return SEC_E_INVALID;
    if (point_pitch < 3) return SEC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (box_counts && (rc = fill_words(box_counts, (size_t)n_boxes * sizeof(int), 0u, st))) return rc;
    if (n_points == 0) return SEC_OK;
    hipLaunchKernelGGL(k_points_in_boxes, dim3(point_blocks(n_points, batch), batch), dim3(kBlock), 0, st, points, point_pitch,
                       point_offsets, boxes, box_offsets, valid, first_box, box_counts);
    return check_launch();
}

SEC_API int sec_noise_per_box_f32(const float *boxes, const int *box_offsets, int n_boxes, int batch, const unsigned char *valid,
                                  const float *loc_noises, const float *rot_noises, int num_try, int max_boxes_per_frame,
                                  int *selected, float *loc_transform, float *rot_transform, void *stream) {
    if (batch <= 0 || n_boxes < 0 || num_try <= 0 || max_boxes_per_frame <= 0 || !box_offsets || !selected || !loc_transform ||
        !rot_transform || (n_boxes > 0 && (!boxes || !loc_noises || !rot_noises)))
        return SEC_E_INVALID;
    if (num_try > kAugMaxTry || max_boxes_per_frame > kAugMaxBoxes) return SEC_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_noise_per_box, dim3(batch), dim3(kBlock), 0, (hipStream_t)stream, boxes, box_offsets, n_boxes, batch, valid,
                       loc_noises, rot_noises, num_try, max_boxes_per_frame, selected, loc_transform, rot_transform);
    return check_launch();
}

SEC_API int sec_augment_points_f32(float *points, int point_pitch, const int *point_offsets, int n_points, int batch,
                                   const int *first_box, const float *boxes, const unsigned char *valid, const float *loc_transform,
                                   const float *rot_transform, const float *frame_params, void *stream) {
    if (batch <= 0 || n_points < 0 || !point_offsets || !frame_params || (n_points > 0 && !points) ||
        (first_box && (!boxes || !loc_transform || !rot_transform)))
        return SEC_E_INVALID;
    if (point_pitch < 3) return SEC_E_UNSUPPORTED;
    if (n_points == 0) return SEC_OK;
    hipLaunchKernelGGL(k_augment_points, dim3(point_blocks(n_points, batch), batch), dim3(kBlock), 0, (hipStream_t)stream, points,
                       point_pitch, point_offsets, first_box, boxes, valid, loc_transform, rot_transform, frame_params);
    return check_launch();
}

static int augment_boxes_impl(const float *boxes, const int *box_offsets, int n_boxes, int batch, const unsigned char *valid,
                              const int *classes, const float *importance, const float *loc_transform, const float *rot_transform,
                              const float *frame_params, const float *h_bev_range4, float *out_boxes, int *out_classes,
                              float *out_importance, int *out_offsets, int box_ndim, void *stream) {
    if (batch <= 0 || n_boxes < 0 || !box_offsets || !frame_params || !h_bev_range4 || !out_offsets || (n_boxes > 0 && (!boxes || !out_boxes)) ||
        (!loc_transform != !rot_transform))
        return SEC_E_INVALID;
    if (box_ndim != 7 && box_ndim != 9) return SEC_E_UNSUPPORTED;       // the reference transforms a velocity only when shape[1] == 9
    hipLaunchKernelGGL(box_ndim == 9 ? k_augment_boxes_velo : k_augment_boxes, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, boxes, box_offsets,
                       n_boxes, batch, valid, classes, importance, loc_transform, rot_transform, frame_params, h_bev_range4[0], h_bev_range4[1],
                       h_bev_range4[2], h_bev_range4[3], out_boxes, out_classes, out_importance, out_offsets);
    return check_launch();
}
SEC_API int sec_augment_boxes_f32(const float *boxes, const int *box_offsets, int n_boxes, int batch, const unsigned char *valid,
                                  const int *classes, const float *importance, const float *loc_transform, const float *rot_transform,
                                  const float *frame_params, const float *h_bev_range4, float *out_boxes, int *out_classes,
                                  float *out_importance, int *out_offsets, void *stream) {
    return augment_boxes_impl(boxes, box_offsets, n_boxes, batch, valid, classes, importance, loc_transform, rot_transform, frame_params,
                              h_bev_range4, out_boxes, out_classes, out_importance, out_offsets, 7, stream);
}
SEC_API int sec_augment_boxes_nd_f32(const float *boxes, const int *box_offsets, int n_boxes, int batch, const unsigned char *valid,
                                     const int *classes, const float *importance, const float *loc_transform, const float *rot_transform,
                                     const float *frame_params, const float *h_bev_range4, int box_ndim, float *out_boxes, int *out_classes,
                                     float *out_importance, int *out_offsets, void *stream) {
    return augment_boxes_impl(boxes, box_offsets, n_boxes, batch, valid, classes, importance, loc_transform, rot_transform, frame_params,
                              h_bev_range4, out_boxes, out_classes, out_importance, out_offsets, box_ndim, stream);
}

SEC_API int sec_db_sample_select_f32(const float *gt_boxes, const int *gt_offsets, int n_gt, int batch, const int *gt_classes,
                                     const unsigned char *gt_valid, const float *gt_importance, const float *db_boxes, int n_db,
                                     const int *candidates, int num_groups, int k, const int *class_of_group, const int *num_table,
                                     int table_len, float sample_importance, int *accepted, int *accepted_count,
                                     int *accepted_per_group, float *out_boxes, int out_capacity, int *out_classes,
                                     unsigned char *out_valid, float *out_importance, unsigned char *out_sampled, int *out_box_offsets,
                                     void *stream) {
    if (batch <= 0 || n_gt < 0 || n_db < 0 || num_groups <= 0 || k <= 0 || table_len <= 0 || out_capacity < 0 || !gt_offsets ||
        !candidates || !class_of_group || !num_table || !accepted || !accepted_count || !accepted_per_group || !out_boxes ||
        !out_box_offsets || (n_gt > 0 && !gt_boxes) || (n_db > 0 && !db_boxes))
        return SEC_E_INVALID;
    if (k > kDbMaxK || num_groups > kDbMaxGroups) return SEC_E_UNSUPPORTED;
    if ((long long)out_capacity < (long long)n_gt + (long long)batch * num_groups * k) return SEC_E_INVALID;   // every frame may accept all
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_db_select, dim3(batch), dim3(kBlock), 0, st, gt_boxes, gt_offsets, n_gt, gt_classes, db_boxes, n_db, candidates,
                       num_groups, k, class_of_group, num_table, table_len, accepted, accepted_count, accepted_per_group);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_db_merge_boxes, dim3(batch), dim3(kBlock), 0, st, gt_boxes, gt_offsets, n_gt, batch, gt_classes, gt_valid,
                       gt_importance, db_boxes, n_db, num_groups, k, class_of_group, sample_importance, accepted, accepted_count,
                       accepted_per_group, out_boxes, out_capacity, out_classes, out_valid, out_importance, out_sampled, out_box_offsets);
    return check_launch();
}

SEC_API size_t sec_db_sample_merge_points_workspace_bytes(int n_points, int batch, int slots) {
    if (n_points < 0 || batch <= 0 || slots <= 0 || slots > kDbMaxK * kDbMaxGroups) return 0;
    return align_up(db_merge_ws_ints(n_points, batch, slots) * sizeof(int));
}

SEC_API int sec_db_sample_merge_points_f32(const float *points, int point_pitch, const int *point_offsets, int n_points, int batch,
                                           const int *first_box, const float *pool_points, const int *pool_offsets,
                                           const float *db_boxes, int n_db, const int *accepted, const int *accepted_count, int slots,
                                           float *out_points, int out_capacity, int *out_point_offsets, int *overflow, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    if (batch <= 0 || n_points < 0 || n_db < 0 || slots <= 0 || out_capacity < 0 || !point_offsets || !accepted || !accepted_count ||
        !out_point_offsets || !overflow || !workspace || (n_points > 0 && !points) || (out_capacity > 0 && !out_points) ||
        (n_db > 0 && (!pool_offsets || !db_boxes)))
        return SEC_E_INVALID;
    if (point_pitch < 3 || slots > kDbMaxK * kDbMaxGroups) return SEC_E_UNSUPPORTED;
    if (workspace_bytes < sec_db_sample_merge_points_workspace_bytes(n_points, batch, slots)) return SEC_E_WORKSPACE;
    if ((long long)div_up(n_points, kBlock) + (long long)batch * slots > 0x7fffffffLL) return SEC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int n_blocks = div_up(n_points, kBlock);
    const DbMergeWs w = db_merge_ws(workspace, n_points, batch, slots);
    int rc;
    if (n_blocks > 0) {
        hipLaunchKernelGGL(k_dbm_count, dim3(n_blocks), dim3(kBlock), 0, st, point_offsets, n_points, batch, first_box, w.blk);
        if ((rc = check_launch())) return rc;
    }
    hipLaunchKernelGGL(k_dbm_scan, dim3(1), dim3(kBlock), 0, st, point_offsets, n_points, batch, first_box, pool_offsets, n_db, accepted,
                       accepted_count, slots, n_blocks, w, out_capacity, out_point_offsets, overflow);
    if ((rc = check_launch())) return rc;
    hipLaunchKernelGGL(k_dbm_scatter, dim3(n_blocks + batch * slots), dim3(kBlock), 0, st, points, point_pitch, point_offsets, n_points,
                       batch, first_box, pool_points, pool_offsets, db_boxes, n_db, accepted, accepted_count, slots, n_blocks, w,
                       out_points, out_capacity);
    return check_launch();
}
