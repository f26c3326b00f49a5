// KITTI annotations from detections on the device: KittiDataset.convert_detection_to_kitti_annos (second/data/kitti_dataset.py:38-107)
// for all images of a val pass at once -- lidar box -> camera box (box_np_ops.box_lidar_to_camera), its eight corners
// (center_to_corner_box3d, origin (0.5, 1.0, 0.5), axis 1), their projection (project_to_image), the image bbox, the drop / clamp rule
// and alpha -- with the kept rows compacted in order.
//
// The detections of all images lie flat in dataset order, image i owns rows [det_off[i], det_off[i + 1]).  Three launches, no host
// read between them:
//   convert   one thread per detection: the reference's float64 operations in its order (the build's -ffp-contract=off keeps every
//             product and sum a separate IEEE operation) into a staging row, the keep flag, and the kept count of each 256 rows;
//   scan      one workgroup: exclusive prefix of the per-256 counts (256 counts per round), then out_off[i] = kept rows in front of
//             det_off[i] -- the flat order is image-major, so the per-image offsets are values of the one flat prefix;
//   scatter   one thread per detection: kept rows move to prefix[row].
// What the reference does that looks like a slip IS the specification: z - h / 2 in float32, zeros (not ones)
// appended before the projection, no clamp behind the camera, np.min / np.max / np.minimum / np.maximum propagate a NaN (fmin / fmax do
// not), the drop rule's comparisons are false for a NaN (such a row is kept), the arc tangent of alpha is a float32 value.
// The inputs are never written (the reference edits the array `.cpu().numpy()` gave it, which for CPU tensors is the caller's).
#include "common.hpp"

namespace sec {

constexpr int kKaStage = 12;          // staging row: bbox 4, alpha, location 3, dimensions 3, rotation_y

struct KaWs { double *stage; signed char *keep; int *blk; };
static KaWs ka_ws(void *ws, int n) {
    KaWs w;
    char *p = (char *)ws;
    const size_t rows = n > 0 ? n : 1;
    w.stage = (double *)p; p += align_up(rows * kKaStage * sizeof(double));
    w.keep = (signed char *)p; p += align_up(rows);
    w.blk = (int *)p;
    return w;
}

// np.min / np.max of two values: a NaN on either side is the result
__device__ __forceinline__ double ka_min(double a, double b) { return (a != a || b != b) ? (a != a ? a : b) : (b < a ? b : a); }
__device__ __forceinline__ double ka_max(double a, double b) { return (a != a || b != b) ? (a != a ? a : b) : (b > a ? b : a); }

// the image that owns flat row i: the first one whose end lies behind i (empty images share their offset with a neighbour)
__device__ __forceinline__ int ka_image_of(const int *__restrict__ det_off, int images, int i) {
    int f0 = 0, f1 = images - 1;
    while (f0 < f1) {
        const int mid = (f0 + f1) >> 1;
        if (det_off[mid + 1] <= i) f0 = mid + 1; else f1 = mid;
    }
    return f0;
}

__global__ __launch_bounds__(kBlock) void k_ka_convert(const float *__restrict__ boxes, const int *__restrict__ det_off, int n, int images,
                                                       const double *__restrict__ lidar2cam, const double *__restrict__ P2,
                                                       const int *__restrict__ image_hw, KaWs w) {
    __shared__ int s_scan[8];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lo = max(det_off[0], 0), hi = min(det_off[images], n);
    int keep = 0;
    if (i < n && i >= lo && i < hi) {
        const int img = ka_image_of(det_off, images, i);
        const float *b = boxes + (size_t)i * 7;
        const float fx = b[0], fy = b[1], fh = b[5];
        const float fz = __fsub_rn(b[2], __fdiv_rn(fh, 2.0f));                   // final_box_preds[:, 2] -= final_box_preds[:, 5] / 2, float32
        const double x = fx, y = fy, z = fz;
        const double *M = lidar2cam + (size_t)img * 16;
        double loc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) loc[r] = M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3] * 1.0;
        const double l = b[4], h = b[5], wd = b[3], ry = b[6];
        const double c = cos(ry), s = sin(ry);
        const double *P = P2 + (size_t)img * 16;
        double mn_u = 0, mn_v = 0, mx_u = 0, mx_v = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // corners_nd: (x, y, z) = bits (4, 2, 1) of k, minus the origin (0.5, 1.0, 0.5), times (l, h, w)
            const double px = l * ((k & 4) ? 0.5 : -0.5), py = h * ((k & 2) ? 0.0 : -1.0), pz = wd * ((k & 1) ? 0.5 : -0.5);
            // einsum('aij,jka->aik') with rot_mat_T = [[c, 0, -s], [0, 1, 0], [s, 0, c]], then + loc
            const double cx = (px * c + py * 0.0 + pz * s) + loc[0];
            const double cy = (px * 0.0 + py * 1.0 + pz * 0.0) + loc[1];
            const double cz = (px * (-s) + py * 0.0 + pz * c) + loc[2];
            // project_to_image: the fourth coordinate is ZERO, the fourth column of P2 takes no part
            const double u = P[0] * cx + P[1] * cy + P[2] * cz;
            const double v = P[4] * cx + P[5] * cy + P[6] * cz;
            const double q = P[8] * cx + P[9] * cy + P[10] * cz;
            const double iu = u / q, iv = v / q;
            if (k == 0) { mn_u = mx_u = iu; mn_v = mx_v = iv; }
            else { mn_u = ka_min(mn_u, iu); mx_u = ka_max(mx_u, iu); mn_v = ka_min(mn_v, iv); mx_v = ka_max(mx_v, iv); }
        }
        const double H = image_hw[2 * img], W = image_hw[2 * img + 1];
        const bool drop = (mn_u > W || mn_v > H) || (mx_u < 0.0 || mx_v < 0.0);  // the written comparisons: false for a NaN
        keep = drop ? 0 : 1;
        double *o = w.stage + (size_t)i * kKaStage;
        o[0] = ka_max(mn_u, 0.0); o[1] = ka_max(mn_v, 0.0); o[2] = ka_min(mx_u, W); o[3] = ka_min(mx_v, H);
        // -np.arctan2(-y, x) on float32 scalars is a float32 value; the sum with rotation_y is float64
        o[4] = (double)(-(float)atan2((double)(-fy), (double)fx)) + ry;
        o[5] = loc[0]; o[6] = loc[1]; o[7] = loc[2];
        o[8] = l; o[9] = h; o[10] = wd; o[11] = ry;
    }
    if (i < n) w.keep[i] = (signed char)keep;
    int total;
    block_exclusive_scan(keep, s_scan, &total);
    if (threadIdx.x == 0) w.blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_ka_scan(const int *__restrict__ det_off, int n, int images, int n_blocks, KaWs w,
                                                    int *__restrict__ out_off) {
    __shared__ int s_scan[8];
    __shared__ int s_all;
    const int tid = threadIdx.x;
    int kept_all = 0;
    for (int c0 = 0; c0 < n_blocks; c0 += kBlock) {
        const int t = c0 + tid;
        int total;
        const int ex = block_exclusive_scan(t < n_blocks ? w.blk[t] : 0, s_scan, &total);
        if (t < n_blocks) w.blk[t] = kept_all + ex;
        kept_all += total;
    }
    if (tid == 0) s_all = kept_all;
    __syncthreads();                                                  // this workgroup's w.blk writes are visible to its own threads
    for (int img = tid; img <= images; img += kBlock) {
        const int p = min(max(det_off[img], 0), n);
        const int t = p / kBlock, r = p % kBlock;
        int before = t < n_blocks ? w.blk[t] : s_all;
        for (int e = 0; e < r; ++e) before += w.keep[t * kBlock + e];   // t * kBlock + r = p <= n: inside the flags
        out_off[img] = before;
    }
}

__global__ __launch_bounds__(kBlock) void k_ka_scatter(const float *__restrict__ scores, const int *__restrict__ labels, int n, KaWs w,
                                                       double *__restrict__ bbox, double *__restrict__ alpha, double *__restrict__ box3d,
                                                       float *__restrict__ score, int *__restrict__ label, int *__restrict__ src) {
    __shared__ int s_scan[8];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int keep = i < n ? w.keep[i] : 0;
    int total;
    const int ex = block_exclusive_scan(keep, s_scan, &total);
    if (!keep) return;
    const int d = w.blk[blockIdx.x] + ex;                             // < n: one slot per kept row in front of this one
    const double *o = w.stage + (size_t)i * kKaStage;
#pragma unroll
    for (int e = 0; e < 4; ++e) bbox[(size_t)d * 4 + e] = o[e];
    alpha[d] = o[4];
#pragma unroll
    for (int e = 0; e < 7; ++e) box3d[(size_t)d * 7 + e] = o[5 + e];
    score[d] = scores[i];
    label[d] = labels[i];
    src[d] = i;
}

}  // namespace sec

using namespace sec;

SEC_API size_t sec_kitti_annos_workspace_bytes(int n) {
    if (n < 0) return 0;
    const size_t rows = n > 0 ? n : 1;
    return align_up(rows * kKaStage * sizeof(double)) + align_up(rows) + align_up((size_t)div_up(rows, kBlock) * sizeof(int)) + 256;
}

SEC_API int sec_kitti_annos_f64(const float *boxes, const float *scores, const int *labels, int n, const int *det_offsets, int images,
                                const double *lidar2cam, const double *P2, const int *image_hw, double *out_bbox, double *out_alpha,
                                double *out_box3d, float *out_score, int *out_label, int *out_src, int *out_offsets, void *workspace,
                                size_t workspace_bytes, void *stream) {
    if (n < 0 || images < 0 || !out_offsets) return SEC_E_INVALID;
    if (images > 0 && (!det_offsets || !lidar2cam || !P2 || !image_hw)) return SEC_E_INVALID;
    if (n > 0 && (!boxes || !scores || !labels || !out_bbox || !out_alpha || !out_box3d || !out_score || !out_label || !out_src))
        return SEC_E_INVALID;
    if (!workspace || workspace_bytes < sec_kitti_annos_workspace_bytes(n)) return SEC_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || images == 0) return fill_words(out_offsets, (size_t)(images + 1) * sizeof(int), 0u, st);
    const KaWs w = ka_ws(workspace, n);
    const int n_blocks = div_up(n, kBlock);
    hipLaunchKernelGGL(k_ka_convert, dim3(n_blocks), dim3(kBlock), 0, st, boxes, det_offsets, n, images, lidar2cam, P2, image_hw, w);
    hipLaunchKernelGGL(k_ka_scan, dim3(1), dim3(kBlock), 0, st, det_offsets, n, images, n_blocks, w, out_offsets);
    hipLaunchKernelGGL(k_ka_scatter, dim3(n_blocks), dim3(kBlock), 0, st, scores, labels, n, w, out_bbox, out_alpha, out_box3d, out_score,
                       out_label, out_src);
    return check_launch();
}
