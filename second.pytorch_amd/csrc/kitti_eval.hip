// KITTI AP evaluation on the device: second/utils/eval.py -- calculate_iou_partly (:362-445), clean_data (:33-89),
// compute_statistics_jit (:182-300), get_thresholds (:12-30) and fused_compute_statistics (:313-359) -- for all images and all
// (class, difficulty, min_overlap) configurations of one eval_class_v3 call (:479-611).
//
// All per-image data is ragged and addressed through int32 prefix offsets [images + 1] (gt rows, dt rows, don't-care rows, and the
// elements of the per-image [dt_i, gt_i] overlap blocks).  A configuration is cfg = (class * num_difficulty + difficulty) * num_k + k;
// cd = cfg / num_k indexes the ignore flags, cfg_min_overlap[cfg] is min_overlaps[k, metric, class].
//
// Stages (each its own entry point; second_amd/kitti_eval.py chains them):
//   overlaps    one launch per metric writes ONLY the per-image diagonal blocks (the reference computes the full matrix of ~75 images
//               against ~75 images per part and slices the blocks out).  Detection-major, as eval_class_v3 calls calculate_iou_partly
//               with dt first: boxes = detections, query boxes = gt.
//   flags       clean_data: one thread per (class x difficulty, row); num_valid_gt by integer atomics.
//   tp scores   compute_statistics_jit(compute_fp=False): one wave per (image chunk, configuration), LANES = DETECTIONS.  The inner
//               loop of the reference is an arg-max over the eligible detections of one gt ("highest score wins, first of equals"):
//               every lane scans its detections j = lane, lane + 64, ... in ascending order with the reference's strict >, a butterfly
//               picks the highest score and among equals the lowest index.  The assigned set is one bit per owned detection in a register.
//   thresholds  get_thresholds: the sequential float64 scan over the descending scores, one lane per configuration.
//   pr          fused_compute_statistics: one wave per (image chunk, configuration), LANE = SCORE THRESHOLD (41 of 64 lanes): the 41
//               recall sample points are independent runs of the same sequential loop over the same image.  Every branch of the
//               candidate rule needs `overlap > min_overlap`, which does not depend on the lane: the wave tests 64 detections of a gt
//               at once (lanes = detections for that moment), ballots the survivors and walks them in ascending order; only then do the
//               lanes diverge on "assigned" / "score < thresh".  An overlap is read exactly once per wave, so the block is not staged;
//               scores, alphas and flags of the image sit in LDS, and so does the per-lane assigned set, as a bitmask [word][lane]
//               (a dynamically indexed register array would live in scratch memory).
//               tp / fp / fn are integers.  The similarity is accumulated per image in gt order, per chunk in image order, and
//               k_ke_pr_reduce adds the chunk partials in chunk order: no floating-point atomics, two runs give identical bits.
#include "common.hpp"
#include "rotated_clip.hpp"

namespace sec {

constexpr int kKeMaxDt = SEC_KITTI_EVAL_MAX_DT, kKeMaxGt = SEC_KITTI_EVAL_MAX_GT, kKePts = SEC_KITTI_EVAL_SAMPLE_PTS;
constexpr int kKeChunk = SEC_KITTI_EVAL_CHUNK;
constexpr int kKeWords = kKeMaxDt / 32;
static_assert(kKeMaxDt % 64 == 0 && kKePts <= kWave, "lanes are detections (tp scores) or thresholds (pr)");

struct KeImage { int g0, ng, d0, nd, o0; bool ok; };
// offsets of image `img`; ok = counts within the caps and every range inside its array (the host refuses what is not, this is the
// second fence: nothing is read or written outside the arrays whatever the offsets hold)
__device__ __forceinline__ KeImage ke_image(const int *__restrict__ gt_off, const int *__restrict__ dt_off, const int *__restrict__ ov_off,
                                            int img, int n_gt, int n_dt, long long n_ov) {
    KeImage m;
    m.g0 = gt_off[img]; m.ng = gt_off[img + 1] - m.g0;
    m.d0 = dt_off[img]; m.nd = dt_off[img + 1] - m.d0;
    m.o0 = ov_off ? ov_off[img] : 0;
    m.ok = m.g0 >= 0 && m.d0 >= 0 && m.o0 >= 0 && m.ng >= 0 && m.nd >= 0 && m.ng <= kKeMaxGt && m.nd <= kKeMaxDt &&
           m.g0 + m.ng <= n_gt && m.d0 + m.nd <= n_dt && (!ov_off || (long long)m.o0 + (long long)m.ng * m.nd <= n_ov);
    return m;
}

// image_box_overlap (eval.py:93-119) for one pair, float64, the same operations in the same order.  criterion -1: IoU, 0: over the
// area of `b`.
__device__ __forceinline__ double ke_image_overlap(const double *__restrict__ b, const double *__restrict__ q, int criterion) {
    const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
    if (!(ih > 0)) return 0.0;
    double ua;
    if (criterion == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih;
    else ua = (b[2] - b[0]) * (b[3] - b[1]);
    return iw * ih / ua;
}

// box_corners of rotated_clip.hpp with the sine and cosine evaluated in float64 and rounded once.  The clipper's intersection points
// (seg_intersect: differences of products of coordinates) are ill-conditioned at KITTI ranges: at 60 m one ulp in a corner moves an
// intersection point by ~1e-4 m and an IoU by ~4e-5, and whether a corner rounds up or down hangs on the last bit of the sine.  The
// reference as the fixture runs it (math.cos / math.sin of the SIMT emulator) multiplies by the correctly rounded values; sinf / cosf
// are 1-2 ulp off.  With the same factors every later operation is the same IEEE float32 operation and the blocks agree with the
// recorded ones far inside the 2e-5 bound.  The arithmetic behind the rounding is box_corners' own, operation for operation.
__device__ __forceinline__ void ke_box_corners(float *c, const float *b) {
    const float ac = (float)cos((double)b[4]), as = (float)sin((double)b[4]);
    const float cx = b[0], cy = b[1], xd = b[2], yd = b[3];
    const float xs[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2};
    const float ys[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = ac * xs[i] + as * ys[i] + cx;
        c[2 * i + 1] = -as * xs[i] + ac * ys[i] + cy;
    }
}

// ---------------------------------------------------------------- overlaps: the [dt_i, gt_i] block of every image
__global__ __launch_bounds__(kBlock) void k_ke_overlaps(int metric, int images, const int *__restrict__ dt_off, const int *__restrict__ gt_off,
                                                       const int *__restrict__ ov_off, const double *__restrict__ dt_boxes,
                                                       const double *__restrict__ gt_boxes, int n_dt, int n_gt, long long n_ov, int z_axis,
                                                       double z_center, double *__restrict__ out) {
    const int a0 = z_axis == 0 ? 1 : 0, a1 = z_axis == 2 ? 1 : 2;         // the two BEV axes: range(3) without z_axis
    for (int img = blockIdx.x; img < images; img += gridDim.x) {
        const KeImage m = ke_image(gt_off, dt_off, ov_off, img, n_gt, n_dt, n_ov);
        if (!m.ok) continue;
        const int pairs = m.nd * m.ng;
        for (int p = threadIdx.x; p < pairs; p += kBlock) {
            const int j = p / m.ng, i = p - j * m.ng;
            double v;
            if (metric == 0) {
                v = ke_image_overlap(dt_boxes + (size_t)(m.d0 + j) * 4, gt_boxes + (size_t)(m.g0 + i) * 4, -1);
            } else {
                const double *b = dt_boxes + (size_t)(m.d0 + j) * 7, *q = gt_boxes + (size_t)(m.g0 + i) * 7;
                // (x, y, w, l, r) of the BEV plane, rounded to float32 as the rotated-IoU entry point receives them
                const float fb[5] = {(float)b[a0], (float)b[a1], (float)b[3 + a0], (float)b[3 + a1], (float)b[6]};
                const float fq[5] = {(float)q[a0], (float)q[a1], (float)q[3 + a0], (float)q[3 + a1], (float)q[6]};
                float c1[8], c2[8];                                        // as k_rotate_iou: c1 = the query box (gt), c2 = the box (dt)
                ke_box_corners(c1, fq);
                ke_box_corners(c2, fb);
                const float ar1 = fq[2] * fq[3], ar2 = fb[2] * fb[3];
                const float in = far_apart(standup_of(c1), standup_of(c2)) ? 0.0f : quad_inter(c1, c2);
                if (metric == 1) {
                    v = (double)(in / (ar1 + ar2 - in));
                } else {                                                   // box3d_overlap_kernel (eval.py:128-164), criterion -1
                    float rinc = in;
                    if (rinc > 0) {
                        const double min_z = fmin(b[z_axis] + b[z_axis + 3] * (1 - z_center), q[z_axis] + q[z_axis + 3] * (1 - z_center));
                        const double max_z = fmax(b[z_axis] - b[z_axis + 3] * z_center, q[z_axis] - q[z_axis + 3] * z_center);
                        const double iw = min_z - max_z;
                        if (iw > 0) {
                            const double area1 = b[3] * b[4] * b[5], area2 = q[3] * q[4] * q[5];
                            const double inc = iw * (double)rinc;
                            const double ua = area1 + area2 - inc;
                            rinc = (float)(inc / ua);                       // the reference stores it back into the float32 array
                        } else {
                            rinc = 0.0f;
                        }
                    }
                    v = (double)rinc;
                }
            }
            out[(size_t)m.o0 + p] = v;
        }
    }
}

// ---------------------------------------------------------------- ignore flags (clean_data)
__constant__ double kKeMinHeight[3] = {40, 25, 25};
__constant__ double kKeMaxOcclusion[3] = {0, 1, 2};
__constant__ double kKeMaxTruncation[3] = {0.15, 0.3, 0.5};
struct KeClassDiff { int name[SEC_KITTI_EVAL_MAX_CD], difficulty[SEC_KITTI_EVAL_MAX_CD]; };

__global__ __launch_bounds__(kBlock) void k_ke_flags(KeClassDiff cds, int ncd, int n_gt, int n_dt, const int *__restrict__ gt_name,
                                                    const double *__restrict__ gt_bbox, const double *__restrict__ gt_occluded,
                                                    const double *__restrict__ gt_truncated, const int *__restrict__ dt_name,
                                                    const double *__restrict__ dt_bbox, signed char *__restrict__ ign_gt,
                                                    signed char *__restrict__ ign_dt, int *__restrict__ num_valid_gt) {
    const int r = blockIdx.x * kBlock + threadIdx.x, cd = blockIdx.y;
    const int cls = cds.name[cd], d = cds.difficulty[cd];
    if (r < n_gt) {
        const int nm = gt_name[r];
        const double height = gt_bbox[(size_t)r * 4 + 3] - gt_bbox[(size_t)r * 4 + 1];
        int valid_class = -1;
        if (nm == cls) valid_class = 1;
        else if (cls == SEC_KITTI_NAME_PEDESTRIAN && nm == SEC_KITTI_NAME_PERSON_SITTING) valid_class = 0;
        else if (cls == SEC_KITTI_NAME_CAR && nm == SEC_KITTI_NAME_VAN) valid_class = 0;
        const bool ignore = gt_occluded[r] > kKeMaxOcclusion[d] || gt_truncated[r] > kKeMaxTruncation[d] || height <= kKeMinHeight[d];
        int f;
        if (valid_class == 1 && !ignore) { f = 0; atomicAdd(&num_valid_gt[cd], 1); }
        else if (valid_class == 0 || (ignore && valid_class == 1)) f = 1;
        else f = -1;
        ign_gt[(size_t)cd * n_gt + r] = (signed char)f;
    }
    if (r < n_dt) {
        const double height = fabs(dt_bbox[(size_t)r * 4 + 3] - dt_bbox[(size_t)r * 4 + 1]);
        int f;
        if (height < kKeMinHeight[d]) f = 1;
        else if (dt_name[r] == cls) f = 0;
        else f = -1;
        ign_dt[(size_t)cd * n_dt + r] = (signed char)f;
    }
}

// ---------------------------------------------------------------- pass 1: the scores of the true positives
__global__ __launch_bounds__(kWave) void k_ke_tp_scores(int images, const int *__restrict__ gt_off, const int *__restrict__ dt_off,
                                                       const int *__restrict__ ov_off, const double *__restrict__ overlaps, long long n_ov,
                                                       const double *__restrict__ dt_score, const signed char *__restrict__ ign_gt,
                                                       const signed char *__restrict__ ign_dt, int n_gt, int n_dt,
                                                       const double *__restrict__ cfg_min_overlap, int num_k,
                                                       double *__restrict__ tp_scores, int *__restrict__ tp_count) {
    const int cfg = blockIdx.x, lane = threadIdx.x, cd = cfg / num_k;
    const double mo = cfg_min_overlap[cfg];
    const double kNoDetection = -10000000.0;
    const int img_end = min(images, ((int)blockIdx.y + 1) * kKeChunk);
    for (int img = blockIdx.y * kKeChunk; img < img_end; ++img) {
        const KeImage m = ke_image(gt_off, dt_off, ov_off, img, n_gt, n_dt, n_ov);
        int cnt = 0;
        if (m.ok) {
            constexpr int kOwn = kKeMaxDt / kWave;         // detections j = lane + 64 * k of this lane
            double sc[kOwn];
            int idt[kOwn];
#pragma unroll
            for (int k = 0; k < kOwn; ++k) {
                const int j = lane + kWave * k;
                const bool on = j < m.nd;
                sc[k] = on ? dt_score[m.d0 + j] : 0.0;
                idt[k] = on ? (int)ign_dt[(size_t)cd * n_dt + m.d0 + j] : -1;
            }
            unsigned assigned = 0u;
            for (int i = 0; i < m.ng; ++i) {
                const int ig = ign_gt[(size_t)cd * n_gt + m.g0 + i];
                if (ig == -1) continue;
                double best = kNoDetection;
                int bidx = 0x7fffffff, bflag = 0;
#pragma unroll
                for (int k = 0; k < kOwn; ++k) {
                    const int j = lane + kWave * k;
                    if (j < m.nd && idt[k] != -1 && !((assigned >> k) & 1u)) {
                        const double ov = overlaps[(size_t)m.o0 + (size_t)j * m.ng + i];
                        if (ov > mo && sc[k] > best) { best = sc[k]; bidx = j; bflag = idt[k]; }
                    }
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const double ob = __shfl_xor(best, d, 64);
                    const int oi = __shfl_xor(bidx, d, 64), of = __shfl_xor(bflag, d, 64);
                    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; bflag = of; }
                }
                if (bidx == 0x7fffffff) continue;            // no detection: a fn, which this pass does not count
                if (!(ig == 1 || bflag == 1)) {              // only a true positive adds a score
                    if (lane == 0) tp_scores[(size_t)cfg * n_gt + m.g0 + cnt] = best;
                    ++cnt;
                }
                if ((bidx & (kWave - 1)) == lane) assigned |= 1u << (bidx >> 6);
            }
        }
        if (lane == 0) tp_count[(size_t)cfg * images + img] = cnt;
    }
}

// ---------------------------------------------------------------- get_thresholds: one lane per configuration
__global__ __launch_bounds__(kWave) void k_ke_thresholds(const double *__restrict__ sorted_scores, long long pitch, const int *__restrict__ n_scores,
                                                        const int *__restrict__ num_valid_gt, int num_k, int configs,
                                                        double *__restrict__ thresholds, int *__restrict__ n_thr) {
    const int cfg = blockIdx.x * kWave + threadIdx.x;
    if (cfg >= configs) return;
    const double *s = sorted_scores + (size_t)cfg * pitch;
    long long n = n_scores[cfg];
    n = n < 0 ? 0 : n > pitch ? pitch : n;
    const double num_gt = (double)num_valid_gt[cfg / num_k];
    double *out = thresholds + (size_t)cfg * kKePts;
    double current_recall = 0.0;
    int nt = 0;
    for (long long i = 0; i < n; ++i) {
        const double l_recall = (double)(i + 1) / num_gt;
        const double r_recall = i < n - 1 ? (double)(i + 2) / num_gt : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
        if (nt < kKePts) out[nt] = s[i];                    // (the reference cannot hold more than 41 either)
        ++nt;
        current_recall += 1 / (kKePts - 1.0);
    }
    nt = nt < kKePts ? nt : kKePts;
    for (int t = nt; t < kKePts; ++t) out[t] = 0.0;
    n_thr[cfg] = nt;
}

// ---------------------------------------------------------------- pass 2: tp / fp / fn / similarity per threshold
__global__ __launch_bounds__(kWave) void k_ke_pr(int images, int configs, const int *__restrict__ gt_off, const int *__restrict__ dt_off,
                                                const int *__restrict__ dc_off, const int *__restrict__ ov_off,
                                                const double *__restrict__ overlaps, long long n_ov, const double *__restrict__ dt_score,
                                                const double *__restrict__ gt_alpha, const double *__restrict__ dt_alpha,
                                                const double *__restrict__ dt_bbox, const double *__restrict__ dc_bbox, int n_dc,
                                                const signed char *__restrict__ ign_gt, const signed char *__restrict__ ign_dt, int n_gt,
                                                int n_dt, const double *__restrict__ cfg_min_overlap, int num_k,
                                                const double *__restrict__ thresholds, const int *__restrict__ n_thr, int metric,
                                                int compute_aos, int *__restrict__ part_cnt, double *__restrict__ part_sim) {
    __shared__ double s_score[kKeMaxDt], s_dalpha[kKeMaxDt], s_galpha[kKeMaxGt];
    __shared__ signed char s_idt[kKeMaxDt], s_igt[kKeMaxGt];
    __shared__ unsigned s_asg[kKeWords][kWave];              // assigned_detection of lane t: bit (j & 31) of s_asg[j >> 5][t]
    const int cfg = blockIdx.x, ch = blockIdx.y, lane = threadIdx.x, cd = cfg / num_k;
    const double mo = cfg_min_overlap[cfg];
    const int nt = min(max(n_thr[cfg], 0), kKePts);
    const bool active = lane < nt;
    const double thresh = active ? thresholds[(size_t)cfg * kKePts + lane] : 0.0;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    const int img_end = min(images, (ch + 1) * kKeChunk);
    for (int img = ch * kKeChunk; img < img_end; ++img) {
        const KeImage m = ke_image(gt_off, dt_off, ov_off, img, n_gt, n_dt, n_ov);
        if (!m.ok) continue;
        __syncthreads();                                      // the previous image is done with the staged arrays
        for (int j = lane; j < m.nd; j += kWave) {
            s_score[j] = dt_score[m.d0 + j];
            s_dalpha[j] = compute_aos ? dt_alpha[m.d0 + j] : 0.0;
            s_idt[j] = ign_dt[(size_t)cd * n_dt + m.d0 + j];
        }
        for (int i = lane; i < m.ng; i += kWave) {
            s_galpha[i] = compute_aos ? gt_alpha[m.g0 + i] : 0.0;
            s_igt[i] = ign_gt[(size_t)cd * n_gt + m.g0 + i];
        }
        const int words = (m.nd + 31) >> 5;
        for (int w = 0; w < words; ++w) s_asg[w][lane] = 0u;
        __syncthreads();
        double sim_img = 0.0;
        for (int i = 0; i < m.ng; ++i) {
            const int ig = s_igt[i];
            if (ig == -1) continue;
            int det_idx = -1;
            bool valid = false, assigned_ignored_det = false;
            double max_overlap = 0.0;
            for (int base = 0; base < m.nd; base += kWave) {
                // lanes are detections here: which of these 64 can take part at all (not flag -1, overlap > min_overlap)?
                const int jl = base + lane;
                const double ovl = jl < m.nd ? overlaps[(size_t)m.o0 + (size_t)jl * m.ng + i] : 0.0;
                unsigned long long cand = __ballot(jl < m.nd && s_idt[jl < m.nd ? jl : 0] != -1 && ovl > mo);
                while (cand) {                                // ... and lanes are thresholds again: the reference's inner loop body
                    const int b = __builtin_ctzll(cand);
                    cand &= cand - 1ull;
                    const int j = base + b;
                    const double overlap = __shfl(ovl, b, 64);
                    const bool taken = (s_asg[j >> 5][lane] >> (j & 31)) & 1u;
                    if (!active || taken || s_score[j] < thresh) continue;
                    const int idj = s_idt[j];
                    if ((overlap > max_overlap || assigned_ignored_det) && idj == 0) {
                        max_overlap = overlap;
                        det_idx = j;
                        valid = true;
                        assigned_ignored_det = false;
                    } else if (!valid && idj == 1) {
                        det_idx = j;
                        valid = true;
                        assigned_ignored_det = true;
                    }
                }
            }
            if (!active) continue;
            if (!valid && ig == 0) {
                ++fn;
            } else if (valid && (ig == 1 || s_idt[det_idx] == 1)) {
                s_asg[det_idx >> 5][lane] |= 1u << (det_idx & 31);
            } else if (valid) {
                ++tp;
                if (compute_aos) sim_img += (1.0 + cos(s_galpha[i] - s_dalpha[det_idx])) / 2.0;
                s_asg[det_idx >> 5][lane] |= 1u << (det_idx & 31);
            }
        }
        // false positives: what is left unassigned, not ignored and above the threshold
        for (int j = 0; j < m.nd; ++j) {
            if (s_idt[j] != 0) continue;
            const bool taken = (s_asg[j >> 5][lane] >> (j & 31)) & 1u;
            if (active && !taken && !(s_score[j] < thresh)) ++fp;
        }
        if (metric == 0 && dc_off) {                          // detections inside DontCare regions are no false positives
            const int c0 = dc_off[img], nc = dc_off[img + 1] - c0;
            if (c0 >= 0 && nc > 0 && c0 + nc <= n_dc) {
                int nstuff = 0;
                for (int i = 0; i < nc; ++i)
                    for (int base = 0; base < m.nd; base += kWave) {
                        const int jl = base + lane;
                        bool c = false;
                        if (jl < m.nd && s_idt[jl] == 0)
                            c = ke_image_overlap(dt_bbox + (size_t)(m.d0 + jl) * 4, dc_bbox + (size_t)(c0 + i) * 4, 0) > mo;
                        unsigned long long cand = __ballot(c);
                        while (cand) {
                            const int j = base + __builtin_ctzll(cand);
                            cand &= cand - 1ull;
                            const bool taken = (s_asg[j >> 5][lane] >> (j & 31)) & 1u;
                            if (!active || taken || s_score[j] < thresh) continue;
                            s_asg[j >> 5][lane] |= 1u << (j & 31);
                            ++nstuff;
                        }
                    }
                fp -= nstuff;
            }
        }
        sim += sim_img;                                       // images in order (a tp == 0 image adds an exact 0)
    }
    if (lane < kKePts) {
        const size_t o = ((size_t)ch * configs + cfg) * kKePts + lane;
        part_cnt[o * 3 + 0] = tp;
        part_cnt[o * 3 + 1] = fp;
        part_cnt[o * 3 + 2] = fn;
        part_sim[o] = sim;
    }
}

__global__ __launch_bounds__(kBlock) void k_ke_pr_reduce(int chunks, int configs, const int *__restrict__ part_cnt,
                                                        const double *__restrict__ part_sim, int *__restrict__ pr_counts,
                                                        double *__restrict__ pr_similarity) {
    const int e = blockIdx.x * kBlock + threadIdx.x;         // (configuration, threshold)
    const int n = configs * kKePts;
    if (e >= n) return;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {                     // chunks in order
        const size_t o = (size_t)ch * n + e;
        tp += part_cnt[o * 3 + 0];
        fp += part_cnt[o * 3 + 1];
        fn += part_cnt[o * 3 + 2];
        sim += part_sim[o];
    }
    pr_counts[(size_t)e * 3 + 0] = tp;
    pr_counts[(size_t)e * 3 + 1] = fp;
    pr_counts[(size_t)e * 3 + 2] = fn;
    pr_similarity[e] = sim;
}

static bool ke_counts_ok(int images, int n_gt, int n_dt, int max_gt, int max_dt) {
    return images >= 0 && n_gt >= 0 && n_dt >= 0 && max_gt >= 0 && max_dt >= 0;
}
static int ke_chunks(int images) { return div_up(images, kKeChunk); }

}  // namespace sec

using namespace sec;

SEC_API int sec_kitti_eval_overlaps(int metric, int images, const int *dt_offsets, const int *gt_offsets, const int *ov_offsets,
                                    const double *dt_boxes, const double *gt_boxes, int n_dt, int n_gt, long long n_ov, int max_dt,
                                    int max_gt, int z_axis, double z_center, double *overlaps, void *stream) {
    if (metric < 0 || metric > 2 || !ke_counts_ok(images, n_gt, n_dt, max_gt, max_dt) || n_ov < 0 || z_axis < 0 || z_axis > 2)
        return SEC_E_INVALID;
    if (images > 0 && (!dt_offsets || !gt_offsets || !ov_offsets)) return SEC_E_INVALID;
    if ((n_dt > 0 && !dt_boxes) || (n_gt > 0 && !gt_boxes) || (n_ov > 0 && !overlaps)) return SEC_E_INVALID;
    if (max_dt > kKeMaxDt || max_gt > kKeMaxGt) return SEC_E_UNSUPPORTED;
    if (images == 0 || n_ov == 0) return SEC_OK;
    hipLaunchKernelGGL(k_ke_overlaps, dim3(images < 65536 ? images : 65536), dim3(kBlock), 0, (hipStream_t)stream, metric, images, dt_offsets,
                       gt_offsets, ov_offsets, dt_boxes, gt_boxes, n_dt, n_gt, n_ov, z_axis, z_center, overlaps);
    return check_launch();
}

SEC_API int sec_kitti_eval_flags(const int *h_class_names, const int *h_difficulties, int num_cd, int n_gt, int n_dt, const int *gt_name,
                                 const double *gt_bbox, const double *gt_occluded, const double *gt_truncated, const int *dt_name,
                                 const double *dt_bbox, signed char *ignored_gt, signed char *ignored_dt, int *num_valid_gt,
                                 void *stream) {
    if (!h_class_names || !h_difficulties || num_cd <= 0 || n_gt < 0 || n_dt < 0 || !num_valid_gt) return SEC_E_INVALID;
    if (n_gt > 0 && (!gt_name || !gt_bbox || !gt_occluded || !gt_truncated || !ignored_gt)) return SEC_E_INVALID;
    if (n_dt > 0 && (!dt_name || !dt_bbox || !ignored_dt)) return SEC_E_INVALID;
    if (num_cd > SEC_KITTI_EVAL_MAX_CD) return SEC_E_UNSUPPORTED;
    KeClassDiff cds;
    for (int i = 0; i < num_cd; ++i) {
        if (h_class_names[i] < 0 || h_class_names[i] > SEC_KITTI_NAME_OTHER || h_difficulties[i] < 0 || h_difficulties[i] > 2)
            return SEC_E_INVALID;
        cds.name[i] = h_class_names[i];
        cds.difficulty[i] = h_difficulties[i];
    }
    for (int i = num_cd; i < SEC_KITTI_EVAL_MAX_CD; ++i) cds.name[i] = cds.difficulty[i] = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = fill_words(num_valid_gt, (size_t)num_cd * sizeof(int), 0u, st))) return rc;
    const int rows = n_gt > n_dt ? n_gt : n_dt;
    if (rows == 0) return SEC_OK;
    hipLaunchKernelGGL(k_ke_flags, dim3(div_up(rows, kBlock), num_cd), dim3(kBlock), 0, st, cds, num_cd, n_gt, n_dt, gt_name, gt_bbox,
                       gt_occluded, gt_truncated, dt_name, dt_bbox, ignored_gt, ignored_dt, num_valid_gt);
    return check_launch();
}

SEC_API int sec_kitti_eval_tp_scores(int images, const int *gt_offsets, const int *dt_offsets, const int *ov_offsets, const double *overlaps,
                                     long long n_ov, const double *dt_score, const signed char *ignored_gt,
                                     const signed char *ignored_dt, int n_gt, int n_dt, int max_gt, int max_dt,
                                     const double *cfg_min_overlap, int num_k, int configs, double *tp_scores, int *tp_count,
                                     void *stream) {
    if (!ke_counts_ok(images, n_gt, n_dt, max_gt, max_dt) || n_ov < 0 || num_k <= 0 || configs <= 0 || configs % num_k || !cfg_min_overlap)
        return SEC_E_INVALID;
    if (images > 0 && (!gt_offsets || !dt_offsets || !ov_offsets || !tp_count)) return SEC_E_INVALID;
    if ((n_ov > 0 && !overlaps) || (n_dt > 0 && (!dt_score || !ignored_dt)) || (n_gt > 0 && (!ignored_gt || !tp_scores)))
        return SEC_E_INVALID;
    if (max_dt > kKeMaxDt || max_gt > kKeMaxGt || configs > 65535) return SEC_E_UNSUPPORTED;
    if (images == 0) return SEC_OK;
    hipLaunchKernelGGL(k_ke_tp_scores, dim3(configs, ke_chunks(images)), dim3(kWave), 0, (hipStream_t)stream, images, gt_offsets, dt_offsets,
                       ov_offsets, overlaps, n_ov, dt_score, ignored_gt, ignored_dt, n_gt, n_dt, cfg_min_overlap, num_k, tp_scores,
                       tp_count);
    return check_launch();
}

SEC_API int sec_kitti_eval_thresholds(const double *sorted_scores, long long pitch, const int *n_scores, const int *num_valid_gt, int num_k,
                                      int configs, double *thresholds, int *n_thresholds, void *stream) {
    if (pitch < 0 || num_k <= 0 || configs <= 0 || configs % num_k || !n_scores || !num_valid_gt || !thresholds || !n_thresholds ||
        (pitch > 0 && !sorted_scores))
        return SEC_E_INVALID;
    hipLaunchKernelGGL(k_ke_thresholds, dim3(div_up(configs, kWave)), dim3(kWave), 0, (hipStream_t)stream, sorted_scores, pitch, n_scores,
                       num_valid_gt, num_k, configs, thresholds, n_thresholds);
    return check_launch();
}

SEC_API size_t sec_kitti_eval_pr_workspace_bytes(int images, int configs) {
    if (images < 0 || configs <= 0) return 0;
    const size_t e = (size_t)(ke_chunks(images) > 0 ? ke_chunks(images) : 1) * configs * kKePts;
    return align_up(e * 3 * sizeof(int)) + align_up(e * sizeof(double)) + 256;
}

SEC_API int sec_kitti_eval_pr(int images, const int *gt_offsets, const int *dt_offsets, const int *dc_offsets, const int *ov_offsets,
                              const double *overlaps, long long n_ov, const double *dt_score, const double *gt_alpha,
                              const double *dt_alpha, const double *dt_bbox, const double *dc_bbox, int n_dc,
                              const signed char *ignored_gt, const signed char *ignored_dt, int n_gt, int n_dt, int max_gt, int max_dt,
                              const double *cfg_min_overlap, int num_k, int configs, const double *thresholds, const int *n_thresholds,
                              int metric, int compute_aos, int *pr_counts, double *pr_similarity, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (!ke_counts_ok(images, n_gt, n_dt, max_gt, max_dt) || n_ov < 0 || n_dc < 0 || num_k <= 0 || configs <= 0 || configs % num_k ||
        metric < 0 || metric > 2 || !cfg_min_overlap || !thresholds || !n_thresholds || !pr_counts || !pr_similarity)
        return SEC_E_INVALID;
    if (images > 0 && (!gt_offsets || !dt_offsets || !ov_offsets)) return SEC_E_INVALID;
    if ((n_ov > 0 && !overlaps) || (n_dt > 0 && (!dt_score || !ignored_dt)) || (n_gt > 0 && !ignored_gt)) return SEC_E_INVALID;
    if (compute_aos && ((n_gt > 0 && !gt_alpha) || (n_dt > 0 && !dt_alpha))) return SEC_E_INVALID;
    if (metric == 0 && n_dc > 0 && (!dc_offsets || !dc_bbox || !dt_bbox)) return SEC_E_INVALID;
    if (max_dt > kKeMaxDt || max_gt > kKeMaxGt || configs > 65535) return SEC_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < sec_kitti_eval_pr_workspace_bytes(images, configs)) return SEC_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = ke_chunks(images);
    Arena ar(workspace, workspace_bytes);
    const size_t e = (size_t)(chunks > 0 ? chunks : 1) * configs * kKePts;
    int *part_cnt = ar.take<int>(e * 3);
    double *part_sim = ar.take<double>(e);
    if (chunks > 0)
        hipLaunchKernelGGL(k_ke_pr, dim3(configs, chunks), dim3(kWave), 0, st, images, configs, gt_offsets, dt_offsets,
                           n_dc > 0 ? dc_offsets : (const int *)nullptr, ov_offsets, overlaps, n_ov, dt_score, gt_alpha, dt_alpha, dt_bbox,
                           dc_bbox, n_dc, ignored_gt, ignored_dt, n_gt, n_dt, cfg_min_overlap, num_k, thresholds, n_thresholds, metric,
                           compute_aos ? 1 : 0, part_cnt, part_sim);
    hipLaunchKernelGGL(k_ke_pr_reduce, dim3(div_up((long long)configs * kKePts, kBlock)), dim3(kBlock), 0, st, chunks, configs, part_cnt,
                       part_sim, pr_counts, pr_similarity);
    return check_launch();
}
