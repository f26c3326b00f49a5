// Training augmentation on the device (include/second_hip.h, "Training augmentation"): what the reference's prep_pointcloud does to one
// frame's points and boxes between loading and voxelising (second/data/preprocess.py:250-286), for a whole batch, without a host read.
//   sec_points_in_boxes_f32  -- box_np_ops.points_in_rbbox / points_count_rbbox (second/core/box_np_ops.py:728-739)
//   sec_noise_per_box_f32    -- preprocess.noise_per_box + _select_transform (second/core/preprocess.py:244-273, 478-484)
//   sec_augment_points_f32   -- points_transform_, random_flip, global_rotation_v2, global_scaling_v2, global_translate_ on the points
//   sec_augment_boxes_f32    -- box3d_transform_ and the same global stages on the boxes, filter_gt_box_outside_range_by_center,
//                               _dict_select (compaction) and limit_period
// Every count (points per frame, boxes per frame, boxes kept) is read from / written to device memory, so the four calls capture
// into a hipGraph.  All arithmetic is plain fp32 (the library builds with -ffp-contract=off and without packed fp32).
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
__global__ __launch_bounds__(kBlock) void k_augment_boxes(const float *__restrict__ boxes, const int *__restrict__ box_offsets, int n_boxes,
                                                          int batch, const unsigned char *__restrict__ valid,
                                                          const int *__restrict__ classes, const float *__restrict__ importance,
                                                          const float *__restrict__ loc_transform,
                                                          const float *__restrict__ rot_transform,
                                                          const float *__restrict__ frame_params, float xmin, float ymin, float xmax,
                                                          float ymax, float *__restrict__ out_boxes, int *__restrict__ out_classes,
                                                          float *__restrict__ out_importance, int *__restrict__ out_offsets) {
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
            int keep = 0;
            if (g < g1) {
                for (int k = 0; k < 7; ++k) v[k] = boxes[(size_t)g * 7 + k];
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
                v[0] = rx * scale + fp[4]; v[1] = ry * scale + fp[5]; v[2] = v[2] * scale + fp[6];       // global_scaling_v2, global_translate_
                v[3] *= scale; v[4] *= scale; v[5] *= scale;
                keep = ok && v[0] > xmin && v[0] < xmax && v[1] > ymin && v[1] < ymax;   // filter_gt_box_outside_range_by_center: the edge is outside
                v[6] = v[6] - floorf(v[6] / (2.0f * kPi) + 0.5f) * (2.0f * kPi);         // limit_period(yaw, 0.5, 2 pi)
            }
            int total;
            const int pos = base + block_exclusive_scan(keep, s_scan, &total);
            if (keep) {
                for (int k = 0; k < 7; ++k) out_boxes[(size_t)pos * 7 + k] = v[k];
                if (out_classes) out_classes[pos] = classes ? classes[g] : 1;
                if (out_importance) out_importance[pos] = importance ? importance[g] : 1.0f;
            }
            base += total;
        }
        if (tid == 0) out_offsets[b + 1] = base;
    }
    for (int g = base + tid; g < n_boxes; g += kBlock) {
        for (int k = 0; k < 7; ++k) out_boxes[(size_t)g * 7 + k] = 0.0f;
        if (out_classes) out_classes[g] = 0;
        if (out_importance) out_importance[g] = 0.0f;
    }
}

// blocks per frame for the two point kernels: the frames' sizes are device data, so the grid is sized for frames of the mean size
// and a grid stride covers the rest
static int point_blocks(int n_points, int batch) {
    const int b = div_up(2LL * div_up(n_points > 0 ? n_points : 1, batch), kBlock);
    return b < 1 ? 1 : (b > 256 ? 256 : b);
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

SEC_API int sec_augment_boxes_f32(const float *boxes, const int *box_offsets, int n_boxes, int batch, const unsigned char *valid,
                                  const int *classes, const float *importance, const float *loc_transform, const float *rot_transform,
                                  const float *frame_params, const float *h_bev_range4, float *out_boxes, int *out_classes,
                                  float *out_importance, int *out_offsets, void *stream) {
    if (batch <= 0 || n_boxes < 0 || !box_offsets || !frame_params || !h_bev_range4 || !out_offsets || (n_boxes > 0 && (!boxes || !out_boxes)) ||
        (!loc_transform != !rot_transform))
        return SEC_E_INVALID;
    hipLaunchKernelGGL(k_augment_boxes, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, boxes, box_offsets, n_boxes, batch, valid, classes,
                       importance, loc_transform, rot_transform, frame_params, h_bev_range4[0], h_bev_range4[1], h_bev_range4[2],
                       h_bev_range4[3], out_boxes, out_classes, out_importance, out_offsets);
    return check_launch();
}
