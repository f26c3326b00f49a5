// Training metrics on the device: VoxelNet.update_metrics (second/pytorch/models/voxelnet.py:654-679) with the modules it calls,
// torchplus/metrics.py Accuracy, PrecisionRecall and two Scalars -- two launches, no host read, no memset.
//
//   count    one thread per anchor (grid-stride): the C logits once -> the largest one that is not a NaN, the class the reference's
//            torch.max picks (lowest index of the maximum; the first NaN if there is one) and the label; 2 + 3 T predicates per
//            anchor, counted per wave with ballot / popcount, per workgroup through LDS, then one int32 atomicAdd per non-zero
//            counter per workgroup.  Integer sums: the result does not depend on the order the workgroups arrive in.
//   finish   one thread: the reference's fp32 arithmetic in its order on the ten state buffers (every count is <= 2^24, so the fp32
//            sums the reference takes over [B, N] are these integers exactly), the returned values, and the counters back to zero
//            for the next call.
// sigmoid is monotone, so the largest logit decides `(sigmoid(x) > t).any()` and `sigmoid(x).max() > t` alike: one sigmoid per
// anchor, 1 / (1 + expf(-x)) in fp32, compared with `>` against the threshold rounded to fp32 (what torch compares a float tensor
// with a Python float as).  NaN: PrecisionRecall takes torch.max of the scores, which is NaN -- false at every threshold; Accuracy
// takes .any() over the classes, where a NaN class is false and the others still count, and its label is torch.max's index, the
// first NaN.  With C = 1 both say "nothing predicted".  DESIGN.md section 9g.
#include "common.hpp"

namespace sec {

constexpr int kTmMaxThr = 16;
constexpr int kTmCounters = 2 + 3 * kTmMaxThr;        // matches, cared, then (tp, fp, fn) per threshold
constexpr int kTmMaxBlocks = 2048;

struct TmThr { float v[kTmMaxThr]; };
struct TmState { float *p[10]; };                     // acc total, count; prec total, count; rec total, count; cls total, count; loc total, count

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

template <typename L>
__global__ __launch_bounds__(kBlock) void k_tm_count(const float *__restrict__ cls, const L *__restrict__ labels,
                                                     const unsigned char *__restrict__ cared, int total, int C, TmThr thr, int T,
                                                     float acc_thr, int *__restrict__ counters) {
    __shared__ int s_cnt[kBlock / kWave][kTmCounters];
    int matches = 0, n_cared = 0;                     // wave-uniform running counts
    int tp[kTmMaxThr], fp[kTmMaxThr], fn[kTmMaxThr];
#pragma unroll
    for (int t = 0; t < kTmMaxThr; ++t) tp[t] = fp[t] = fn[t] = 0;
    const int stride = gridDim.x * kBlock;
    // every wave runs the same number of rounds with all 64 lanes (the ballots want them); lanes past the end count nothing
    for (int base = blockIdx.x * kBlock; base < total; base += stride) {
        const int i = base + threadIdx.x;
        const bool live = i < total;
        float m = -INFINITY;                           // largest logit that is not a NaN
        int arg = -1, first_nan = -1;                  // its lowest index (-1: the row has none); the first NaN
        long long label = -1;
        bool w = false;
        if (live) {
            const float *row = cls + (size_t)i * C;
            for (int c = 0; c < C; ++c) {
                const float x = row[c];
                if (x != x) { if (first_nan < 0) first_nan = c; }
                else if (arg < 0 || x > m) { m = x; arg = c; }
            }
            label = (long long)labels[i];
            w = cared ? cared[i] != 0 : label >= 0;
        }
        const float score = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-m)));       // m = -inf: 1 / inf = 0
        const bool acc_any = arg >= 0 && score > acc_thr;
        const long long pred = acc_any ? (first_nan >= 0 ? first_nan : arg) + 1 : 0;
        matches += wave_count(live && pred == label);
        n_cared += wave_count(w);
        const bool pos = w && label > 0, neg = w && label == 0;
        const bool pr_ok = live && first_nan < 0;      // torch.max over the scores of a row with a NaN is NaN
#pragma unroll
        for (int t = 0; t < kTmMaxThr; ++t) {
            if (t < T) {
                const bool hit = pr_ok && score > thr.v[t];
                tp[t] += wave_count(pos && hit);
                fp[t] += wave_count(neg && hit);
                fn[t] += wave_count(pos && !hit);
            }
        }
    }
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_cnt[wave][0] = matches;
        s_cnt[wave][1] = n_cared;
#pragma unroll
        for (int t = 0; t < kTmMaxThr; ++t) {
            s_cnt[wave][2 + 3 * t] = tp[t];
            s_cnt[wave][3 + 3 * t] = fp[t];
            s_cnt[wave][4 + 3 * t] = fn[t];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 + 3 * T) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < kBlock / kWave; ++k) v += s_cnt[k][threadIdx.x];
        if (v) atomicAdd(&counters[threadIdx.x], v);
    }
}

__global__ void k_tm_finish(int *__restrict__ counters, int T, const float *__restrict__ cls_loss, const float *__restrict__ loc_loss,
                            TmState s, float *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // Accuracy.forward: count += clamp(sum(weights), min=1), total += sum(pred == label) over ALL anchors
    const float n_cared = (float)counters[1];
    *s.p[1] = __fadd_rn(*s.p[1], n_cared < 1.0f ? 1.0f : n_cared);
    *s.p[0] = __fadd_rn(*s.p[0], (float)counters[0]);
    out[0] = __fdiv_rn(*s.p[0], *s.p[1]);
    // PrecisionRecall.forward: each pair moves only when its own denominator of this call is positive
    for (int t = 0; t < T; ++t) {
        const float tp = (float)counters[2 + 3 * t], fp = (float)counters[3 + 3 * t], fn = (float)counters[4 + 3 * t];
        const float rec_count = __fadd_rn(tp, fn), prec_count = __fadd_rn(tp, fp);
        if (rec_count > 0.0f) {
            s.p[5][t] = __fadd_rn(s.p[5][t], rec_count);
            s.p[4][t] = __fadd_rn(s.p[4][t], tp);
        }
        if (prec_count > 0.0f) {
            s.p[3][t] = __fadd_rn(s.p[3][t], prec_count);
            s.p[2][t] = __fadd_rn(s.p[2][t], tp);
        }
        const float pc = s.p[3][t], rc = s.p[5][t];
        out[5 + t] = __fdiv_rn(s.p[2][t], pc < 1.0f ? 1.0f : pc);
        out[5 + T + t] = __fdiv_rn(s.p[4][t], rc < 1.0f ? 1.0f : rc);
    }
    // Scalar.forward: `if not scalar.eq(0.0)` -- a NaN loss is not equal to zero and is added; total / count is NaN until the
    // first non-zero loss
    const float cl = *cls_loss, ll = *loc_loss;
    if (!(cl == 0.0f)) { *s.p[7] = __fadd_rn(*s.p[7], 1.0f); *s.p[6] = __fadd_rn(*s.p[6], cl); }
    if (!(ll == 0.0f)) { *s.p[9] = __fadd_rn(*s.p[9], 1.0f); *s.p[8] = __fadd_rn(*s.p[8], ll); }
    out[1] = __fdiv_rn(*s.p[6], *s.p[7]);
    out[2] = cl;
    out[3] = __fdiv_rn(*s.p[8], *s.p[9]);
    out[4] = ll;
    for (int k = 0; k < 2 + 3 * T; ++k) counters[k] = 0;
}

}  // namespace sec

using namespace sec;

SEC_API size_t sec_train_metrics_workspace_bytes(int num_thresholds) {
    if (num_thresholds < 0 || num_thresholds > kTmMaxThr) return 0;
    return align_up(kTmCounters * sizeof(int));
}

SEC_API int sec_train_metrics_f32(const float *cls_preds, const void *labels, int labels_are_i64, const unsigned char *cared,
                                  long long num_anchors, int num_class, const float *h_thresholds, int num_thresholds,
                                  float acc_threshold, const float *cls_loss, const float *loc_loss, float *const *h_state10, float *out,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    if (!h_state10 || !out || !cls_loss || !loc_loss || num_thresholds < 0 || num_anchors < 0 || num_class < 1) return SEC_E_INVALID;
    for (int k = 0; k < 10; ++k)
        if (!h_state10[k]) return SEC_E_INVALID;
    if (num_thresholds > kTmMaxThr || num_anchors > (1ll << 24)) return SEC_E_UNSUPPORTED;
    if ((num_thresholds > 0 && !h_thresholds) || (num_anchors > 0 && (!cls_preds || !labels))) return SEC_E_INVALID;
    if (!workspace || workspace_bytes < sec_train_metrics_workspace_bytes(num_thresholds)) return SEC_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    TmThr thr;
    for (int t = 0; t < kTmMaxThr; ++t) thr.v[t] = t < num_thresholds ? h_thresholds[t] : INFINITY;
    TmState s;
    for (int k = 0; k < 10; ++k) s.p[k] = h_state10[k];
    int *counters = (int *)workspace;
    const int total = (int)num_anchors;
    const int blocks = total > 0 ? (div_up(total, kBlock) < kTmMaxBlocks ? div_up(total, kBlock) : kTmMaxBlocks) : 1;
    if (labels_are_i64)
        hipLaunchKernelGGL(k_tm_count<long long>, dim3(blocks), dim3(kBlock), 0, st, cls_preds, (const long long *)labels, cared, total,
                           num_class, thr, num_thresholds, acc_threshold, counters);
    else
        hipLaunchKernelGGL(k_tm_count<int>, dim3(blocks), dim3(kBlock), 0, st, cls_preds, (const int *)labels, cared, total, num_class,
                           thr, num_thresholds, acc_threshold, counters);
    hipLaunchKernelGGL(k_tm_finish, dim3(1), dim3(kWave), 0, st, counters, num_thresholds, cls_loss, loc_loss, s, out);
    return check_launch();
}
