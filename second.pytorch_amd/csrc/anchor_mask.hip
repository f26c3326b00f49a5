// Anchor-area mask of the KITTI PointPillars configs (`anchor_area_threshold: 1`) on the device.
//
// The reference computes it per frame in its DataLoader workers (second/data/preprocess.py:345-357):
//   dense  = sparse_sum_for_anchors_mask(coors, (ny, nx))       box_np_ops.py:917-922  voxels per BEV cell
//   dense  = dense.cumsum(0).cumsum(1)                           inclusive 2-D prefix sums
//   bv     = rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]])   box_np_ops.py:286-298  (near_bbox() of common.hpp)
//   area   = fused_get_anchors_area(dense, bv, voxel_size, pc_range, grid_size)   box_np_ops.py:925-946
//   mask   = area > anchor_area_threshold
// and uses it to drop anchors before the score threshold of VoxelNet.predict (voxelnet.py:397-439) and to prune the anchors of
// the target assignment (target_ops.py:71-81, 208-215).
//
// What is reproduced EXACTLY, because the mask flips on it:
//   * the cell indices are float32: c = floorf((e - offset) / voxel_size), one IEEE subtraction and one IEEE division, no
//     reciprocal, no contraction, no float64.  On the xyres_16 geometry the quotients are integers in real arithmetic, and
//     float32 / float64 disagree on the floor for a third of the columns;
//   * area = D[c3, c2] - D[c3, c0] - D[c1, c2] + D[c1, c0] with c0 / c1 the MIN cell itself -- the row and the column of the
//     min cell are excluded.  That is the reference's arithmetic, not the textbook integral-image formula (which would read
//     c0 - 1 / c1 - 1), and it is kept;
//   * the reference clamps c0, c1 from below and c2, c3 from above only.  Here every index is clamped to the map on both sides, so
//     no index leaves it; wherever the reference's own indexing is defined (no negative wrap-around, no out-of-bounds read) the two
//     agree.
// Counts and prefix sums are int32 (the reference's float32 sums are integers below 2^24: identical values), so the result does not
// depend on the order of the atomics.
//
// Launches (all on the caller's stream, no host read, capturable): clear | one thread per voxel row, non-returning atomicAdd |
// row scan, one wave per map row | column scan, 64 columns x 16 row segments per workgroup, segment totals through LDS (one latency
// round instead of a chain of `ny` dependent loads) | one thread per anchor, indices computed once, loop over the frames.
#include "common.hpp"

namespace sec {

__global__ __launch_bounds__(kBlock) void k_am_count(const int *__restrict__ coords, int rows_cap, const int *__restrict__ num_dev,
                                                    int batch, int gy, int gx, int *__restrict__ cnt) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int n = rows_cap;
    if (num_dev) n = min(max(*num_dev, 0), rows_cap);
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4 *>(coords)[i];        // (b, z, y, x)
    if ((unsigned)c.x >= (unsigned)batch || (unsigned)c.z >= (unsigned)gy || (unsigned)c.w >= (unsigned)gx) return;
    atomicAdd(&cnt[((size_t)c.x * gy + c.z) * gx + c.w], 1);
}

// inclusive scan along x: one wave per (frame, row)
__global__ __launch_bounds__(kBlock) void k_am_scan_rows(int *__restrict__ cnt, long long n_rows, int gx) {
    const long long r = (long long)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    int *row = cnt + r * gx;
    const int lane = lane_id();
    int carry = 0;
    for (int x0 = 0; x0 < gx; x0 += kWave) {
        const int x = x0 + lane;
        const int v = x < gx ? row[x] : 0;
        const int inc = wave_inclusive_scan(v) + carry;
        if (x < gx) row[x] = inc;
        carry = __shfl(inc, 63, 64);
    }
}

// inclusive scan along y: a workgroup owns 64 columns of one frame; wave s scans rows [s * seg, (s + 1) * seg) of them
constexpr int kAmSegs = 16;
__global__ __launch_bounds__(kAmSegs * kWave) void k_am_scan_cols(int *__restrict__ cnt, int gy, int gx) {
    __shared__ int s_tot[kAmSegs][kWave];
    const int lane = lane_id(), s = threadIdx.x >> 6;
    const int x = blockIdx.x * kWave + lane;
    const int seg = (gy + kAmSegs - 1) / kAmSegs;
    const int y0 = min(s * seg, gy), y1 = min(y0 + seg, gy);
    int *col = cnt + (size_t)blockIdx.y * gy * gx + (x < gx ? x : 0);
    const bool on = x < gx;
    int tot = 0;
    for (int y = y0; y < y1; ++y) tot += ld_sel(col, (size_t)y * gx, on, 0);     // independent loads, one add each
    s_tot[s][lane] = tot;
    __syncthreads();
    int run = 0;
    for (int i = 0; i < s; ++i) run += s_tot[i][lane];
    if (!on) return;
    for (int y = y0; y < y1; ++y) {
        run += col[(size_t)y * gx];
        col[(size_t)y * gx] = run;
    }
}

__global__ __launch_bounds__(kBlock) void k_am_mask(const int *__restrict__ D, int batch, int gy, int gx,
                                                   const float *__restrict__ anchors, int n_anchor, float vx, float vy, float ox,
                                                   float oy, float threshold, unsigned char *__restrict__ mask) {
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= n_anchor) return;
    const float *p = anchors + (size_t)a * 7;
    const float4 bv = near_bbox(p[0], p[1], p[3], p[4], p[6]);
    // float32, one subtraction and one division each, then floor; clamped to the map while still a float (a NaN becomes 0)
    const float fx = (float)(gx - 1), fy = (float)(gy - 1);
    const int c0 = (int)fminf(fmaxf(floorf(__fdiv_rn(__fsub_rn(bv.x, ox), vx)), 0.0f), fx);
    const int c1 = (int)fminf(fmaxf(floorf(__fdiv_rn(__fsub_rn(bv.y, oy), vy)), 0.0f), fy);
    const int c2 = (int)fminf(fmaxf(floorf(__fdiv_rn(__fsub_rn(bv.z, ox), vx)), 0.0f), fx);
    const int c3 = (int)fminf(fmaxf(floorf(__fdiv_rn(__fsub_rn(bv.w, oy), vy)), 0.0f), fy);
    const size_t iD = (size_t)c3 * gx + c2, iA = (size_t)c1 * gx + c0, iB = (size_t)c3 * gx + c0, iC = (size_t)c1 * gx + c2;
    for (int b = 0; b < batch; ++b) {
        const int *Db = D + (size_t)b * gy * gx;
        const int area = Db[iD] - Db[iB] - Db[iC] + Db[iA];
        mask[(size_t)b * n_anchor + a] = (float)area > threshold ? 1 : 0;
    }
}

}  // namespace sec

using namespace sec;

SEC_API size_t sec_anchor_area_mask_workspace_bytes(int batch, int grid_y, int grid_x) {
    if (batch <= 0 || grid_y <= 0 || grid_x <= 0) return 0;
    const unsigned long long cells = (unsigned long long)batch * (unsigned long long)grid_y * (unsigned long long)grid_x;
    if (cells > 0x1fffffffull) return 0;                    // the map is cleared in 32-bit words counted in an int
    return align_up((size_t)cells * sizeof(int)) + 256;
}

SEC_API int sec_anchor_area_mask(const int *coords, int rows_cap, const int *num_dev, int batch, int grid_y, int grid_x,
                                 const float *anchors, int n_anchor, const float *h_voxel_size2, const float *h_offset2,
                                 float threshold, unsigned char *mask, void *workspace, size_t workspace_bytes, void *stream) {
    if (!mask || !anchors || !h_voxel_size2 || !h_offset2 || rows_cap < 0 || (rows_cap > 0 && !coords) || batch <= 0 || grid_y <= 0 ||
        grid_x <= 0 || n_anchor <= 0)
        return SEC_E_INVALID;
    if (!(h_voxel_size2[0] > 0.0f) || !(h_voxel_size2[1] > 0.0f) || !(threshold >= 0.0f)) return SEC_E_INVALID;
    const size_t need = sec_anchor_area_mask_workspace_bytes(batch, grid_y, grid_x);
    if (need == 0) return SEC_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < need) return SEC_E_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const size_t cells = (size_t)batch * grid_y * grid_x;
    int *cnt = ar.take<int>(cells);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = fill_words(cnt, cells * sizeof(int), 0u, st))) return rc;       // (a kernel: this runs inside captured steps)
    if (rows_cap > 0)
        hipLaunchKernelGGL(k_am_count, dim3(div_up(rows_cap, kBlock)), dim3(kBlock), 0, st, coords, rows_cap, num_dev, batch, grid_y,
                           grid_x, cnt);
    const long long n_rows = (long long)batch * grid_y;
    hipLaunchKernelGGL(k_am_scan_rows, dim3(div_up(n_rows, kBlock / kWave)), dim3(kBlock), 0, st, cnt, n_rows, grid_x);
    hipLaunchKernelGGL(k_am_scan_cols, dim3(div_up(grid_x, kWave), batch), dim3(kAmSegs * kWave), 0, st, cnt, grid_y, grid_x);
    hipLaunchKernelGGL(k_am_mask, dim3(div_up(n_anchor, kBlock)), dim3(kBlock), 0, st, cnt, batch, grid_y, grid_x, anchors, n_anchor,
                       h_voxel_size2[0], h_voxel_size2[1], h_offset2[0], h_offset2[1], threshold, mask);
    return check_launch();
}
