// PointPillars front end + NuScenes block filter on gfx950.
//   sec_pfn_kind_fwd           : PillarFeatureNet.forward with one PFNLayer, eval mode
//                                (second/pytorch/models/pointpillars.py:203-237 + :51-65): ~15 torch kernels on a
//                                [P,60,9] tensor in the reference, ONE launch here.  One wave64 per pillar, lane =
//                                output channel (64 channels == one wave), points broadcast with v_readlane.
//                                (kind, with_distance) name one of the four encoders of that file, each with the
//                                optional distance entry (pfn_row).
//   sec_pfn_kind_fwd_slots     : the same from the voxeliser's point lists, no [P,T,4] tensor
//   sec_pfn_kind_train_fwd/bwd : the layer under train() (batch statistics, backward through the argmax), five kernels;
//                                num_dev: static capacity with the pillar count on the device
//   sec_pfn_fwd, sec_pfn_radius_*, their _slots, _train_ and _live forms: the same launchers with the kind fixed by the
//                                name (PLAIN / RADIUS without distance); see "host side" below
//   sec_voxel_block_filter_f32 : height-span filter of points_to_voxel_3d_with_filtering (SURVEY A.2,
//                                enabled by second/configs/nuscenes/all.fhd.config:9-12) + order-preserving
//                                compaction of the voxel arrays (flag + exclusive scan).
#include "common.hpp"

namespace sec {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <typename OT> __device__ __forceinline__ OT cvt_out(float v);
template <> __device__ __forceinline__ float cvt_out(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 cvt_out(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ __half cvt_out(float v) { return __float2half_rn(v); }

// The decorated row of one point, shared by inference (k_pfn_fwd) and the training kernels below, so that both evaluate the very
// same expressions (the library is built with -ffp-contract=off: the radius is multiply, multiply, add, square root, each correctly
// rounded).  The four encoders of pointpillars.py by KIND (SEC_PFN_*), m = cluster mean, c = pillar centre, both Cartesian in all:
//   kPfnPlain         [x, y, z, w, x - mx, y - my, z - mz, x - cx, y - cy]            (9)
//   kPfnRadius        [r, z, w, x - mx, y - my, z - mz, x - cx, y - cy]               (8)  r = sqrt(x * x + y * y)
//   kPfnOld           [x - cx, y - cy, z, w, x - mx, y - my, z - mz, x - cx, y - cy]  (9)  the reference writes the centre offsets
//                     through a view into the raw x, y columns AFTER it took the mean: columns 0, 1 repeat columns 7, 8 bit for bit
//   kPfnRadiusHeight  [r, z, w, x - mx, y - my, z - mz, x - cx, y - cy, h]            (9)  h = max z - min z over the pillar's T slots
// DIST (with_distance) appends sqrt(a * a + b * b + z * z) over the first three feature columns as the reference holds them at that
// point: raw x, y, z, and for kPfnOld the centred x - cx, y - cy with raw z; it comes last (after h): three products, the adds left
// to right, the square root.
enum { kPfnPlain = SEC_PFN_PLAIN, kPfnRadius = SEC_PFN_RADIUS, kPfnOld = SEC_PFN_OLD, kPfnRadiusHeight = SEC_PFN_RADIUS_HEIGHT };
constexpr int pfn_width(int kind, bool dist) { return (kind == kPfnRadius ? 8 : 9) + (dist ? 1 : 0); }
template <int KIND, bool DIST>
__device__ __forceinline__ void pfn_row(const float4 q, float mx, float my, float mz, float cx, float cy, float h,
                                        float (&f)[pfn_width(KIND, DIST)]) {
    constexpr bool POLAR = KIND == kPfnRadius || KIND == kPfnRadiusHeight;
    constexpr int B = POLAR ? 3 : 4;                  // the raw part's width
    if constexpr (POLAR) {
        f[0] = __fsqrt_rn(__fadd_rn(__fmul_rn(q.x, q.x), __fmul_rn(q.y, q.y)));
        f[1] = q.z; f[2] = q.w;
    } else {
        f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    }
    f[B] = q.x - mx; f[B + 1] = q.y - my; f[B + 2] = q.z - mz; f[B + 3] = q.x - cx; f[B + 4] = q.y - cy;
    if constexpr (KIND == kPfnOld) { f[0] = f[B + 3]; f[1] = f[B + 4]; }       // the centred columns stand where raw x, y stood
    if constexpr (KIND == kPfnRadiusHeight) f[B + 5] = h;
    if constexpr (DIST) {
        const float a = KIND == kPfnOld ? f[0] : q.x, b = KIND == kPfnOld ? f[1] : q.y;
        f[pfn_width(KIND, DIST) - 1] =
            __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(q.z, q.z)));
    }
}
// h of kPfnRadiusHeight: the wave's max z - min z.  A lane holds the extrema of the slots it read (a padded slot's zero z among them,
// as the reference's min / max over the whole tensor has it) or the identities +inf / -inf when it read none (lanes >= T).
__device__ __forceinline__ float wave_span(float lo, float hi) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    }
    return __fsub_rn(hi, lo);
}

// F = 4 point features (x, y, z, r/dt), IN = 9 decorated features
// SLOTS: `voxels` is the caller's flat POINT array and `slots` the voxeliser's point lists (slots[p * T + t] = index of pillar p's
// t-th point, vox_slots_of): the pillar's points are fetched through the list instead of from a [P, T, 4] tensor -- the same
// values in the same positions (slots >= n read as zero), so the result is bit-identical, and the voxeliser need not write (nor
// this kernel re-read) that tensor: 98 MB each way at 100 k pillars x 60 slots.
// KIND / DIST: the decorated row of pfn_row (kPfnRadius: the raw x, y give way to their radius, in the arithmetic store_radius_row4
// pins to torch.norm); the cluster mean and the pillar centre stay Cartesian, as above.  kPfnRadiusHeight takes min / max z in the
// mean pass, over the same T slots (SLOTS: the slots >= n read as zero there too).
template <typename OT, bool SLOTS = false, int KIND = kPfnPlain, bool DIST = false>
__global__ __launch_bounds__(kBlock) void k_pfn_fwd(const float *__restrict__ voxels, const int *__restrict__ num_points,
                                                   const int *__restrict__ coords, int P, const int *__restrict__ num_dev,
                                                   int T, const float *__restrict__ wt, const float *__restrict__ scale,
                                                   const float *__restrict__ shift, int C, float vx, float vy, float xo,
                                                   float yo, OT *__restrict__ out, const int *__restrict__ slots = nullptr) {
    if (num_dev) P = *num_dev < P ? *num_dev : P;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (p >= P) return;
    const float4 *pv = reinterpret_cast<const float4 *>(voxels) + (SLOTS ? (size_t)0 : (size_t)p * T);
    const int *sl = SLOTS ? slots + (size_t)p * T : nullptr;
    const int n = num_points[p];
    const int4 co = *reinterpret_cast<const int4 *>(coords + (size_t)p * 4);
    const float cx = __fadd_rn(__fmul_rn((float)co.w, vx), xo), cy = __fadd_rn(__fmul_rn((float)co.z, vy), yo);
    // pillar mean over all T slots (padded slots are zero) / n
    float sx = 0.f, sy = 0.f, sz = 0.f;
    float4 mine = make_float4(0, 0, 0, 0);            // T <= 64: lane t keeps point t for the channel loop below
    float zlo = INFINITY, zhi = -INFINITY;
    for (int t0 = 0; t0 < T; t0 += 64) {
        float4 q = make_float4(0, 0, 0, 0);
        if (t0 + lane < T) {
            if (SLOTS) { if (t0 + lane < n) q = pv[sl[t0 + lane]]; }
            else q = pv[t0 + lane];
            if constexpr (KIND == kPfnRadiusHeight) { zlo = fminf(zlo, q.z); zhi = fmaxf(zhi, q.z); }
        }
        if (t0 == 0) mine = q;
        sx += q.x; sy += q.y; sz += q.z;
    }
    const float inv = (float)n;
    const float mx = wave_sum(sx) / inv, my = wave_sum(sy) / inv, mz = wave_sum(sz) / inv;
    float h = 0.f;
    if constexpr (KIND == kPfnRadiusHeight) h = wave_span(zlo, zhi);
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const bool live = c < C;
        constexpr int IN = pfn_width(KIND, DIST);
        float w[IN];
#pragma unroll
        for (int j = 0; j < IN; ++j) w[j] = live ? wt[(size_t)j * C + c] : 0.f;
        const float sc = live ? scale[c] : 0.f, sh = live ? shift[c] : 0.f;
        float best = (n < T) ? fmaxf(sh, 0.f) : -INFINITY;   // padded slots: relu(bn(linear(0)))
        for (int t = 0; t < n && t < T; ++t) {
            // SLOTS, T <= 64 (every shipped config): the point sits in lane t's registers since the mean pass -- four v_readlane
            // instead of a doubly dependent broadcast load (slot index, then point) per point: 105 -> 78 us at 100 k pillars
            float4 q;
            if (SLOTS && T <= 64) {                       // (the tensor form is 4 us FASTER with its plain broadcast loads: 68 vs 73 us)
                q.x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.x), t));
                q.y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.y), t));
                q.z = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.z), t));
                q.w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.w), t));
            } else {
                q = SLOTS ? pv[sl[t]] : pv[t];            // wave-uniform address: one broadcast load
            }
            float f[IN];
            pfn_row<KIND, DIST>(q, mx, my, mz, cx, cy, h, f);
            float y = 0.f;
#pragma unroll
            for (int j = 0; j < IN; ++j) y = fmaf(f[j], w[j], y);
            y = fmaxf(fmaf(y, sc, sh), 0.f);
            best = fmaxf(best, y);
        }
        if (live) out[(size_t)p * C + c] = cvt_out<OT>(best);
    }
}

// ---- PillarFeatureNet in TRAINING mode: batch statistics, forward and backward -------------------------------------------
// Reference: PFNLayer.forward (pointpillars.py:51-65) under train(): x = Linear(9, C, bias=False)(decorated, masked points);
// BatchNorm1d over ALL P * T rows (the zero rows of the padded slots included), ReLU, max over the T slots; autograd then runs
// ~25 kernels over a [P, T, C] tensor (1.1 GB in fp32 at 75 k pillars x 60 points x 64 channels) forward and again backward.
// Here the [P, T, C] tensor never exists: lane = channel, a wave walks the points of a pillar.
//   k_pfn_stats     per channel: sum x, sum x^2 (both accumulated in fp64, see there), M[c][j] = sum x_c * dec_j, and
//                   S1[j] = sum dec_j (block partials)
//   k_pfn_finalize  mean, 1 / sqrt(var + eps) (biased variance over P * T rows, as BatchNorm does), running statistics
//   k_pfn_fwd<.., TRAIN>  normalise, ReLU, max over the slots, slot of the maximum (-1: a padded slot won)
//   k_pfn_bwd       the gradient of the max reaches ONE row per (pillar, channel): dz = g * [out > 0]; block partials of
//                   dbeta = sum dz, dgamma = sum dz * xhat, A[c][j] = sum dz * dec_j over those rows
//   k_pfn_bwd_finalize  BatchNorm's backward spreads dbeta / dgamma over every row (dx = gamma * invstd * (dz - dbeta / N -
//                   xhat * dgamma / N)); summed against the inputs that is closed form in S1 and M:
//                   dW[c][j] = gamma_c invstd_c (A[c][j] - dbeta_c / N * S1[j] - dgamma_c / N * invstd_c (M[c][j] - mean_c S1[j]))
// No gradient with respect to the points (they are data).
// KIND / DIST (the other encoders of pointpillars.py under train()): the same five kernels on the K-entry row of pfn_row<KIND, DIST>;
// a padded slot is zero in all K entries (the reference masks after decorating, h and the distance included), so it is the same
// x = 0 row as above.
constexpr int kPfnIn = 9;                         // sec_pfn_train_workspace_bytes' row width (see pfn_train_ws_width)
template <int KIND, bool DIST> struct PfnDims {
    static constexpr int K = pfn_width(KIND, DIST);   // decorated inputs
    static constexpr int StatVals = 2 + K;        // per channel: sum x, sum x^2, M[c][0..K-1]
    static constexpr int BwdVals = 2 + K;         // per channel: dbeta, dgamma, A[c][0..K-1]
};
constexpr int kPfnMaxBlocks = 1024;

struct PfnPillar {
    float mx, my, mz, cx, cy, h;
    int n;
};
// Static capacity (the *_live entry points): the arrays hold P rows, of which the first min(max(*num_dev, 0), P) are pillars; the
// count lives in device memory, so a captured graph replays on whatever the voxeliser counted.  One wave-uniform load, kept in a
// scalar register; num_dev == NULL: all P rows are pillars.  Rows at or past the count are never read by any kernel below.
__device__ __forceinline__ int pfn_live(const int *__restrict__ num_dev, int P) {
    if (!num_dev) return P;
    int v = __builtin_amdgcn_readfirstlane(*num_dev);
    v = v > 0 ? v : 0;
    return v < P ? v : P;
}
// the pillar constants exactly as k_pfn_fwd derives them (mean over all T slots / n, pillar centre from its coordinates, and for
// kPfnRadiusHeight max z - min z over the T slots; h = 0 and no work for it otherwise)
template <int KIND>
__device__ __forceinline__ PfnPillar pfn_pillar(const float4 *__restrict__ pv, int T, int n, const int *__restrict__ coords, int p,
                                                float vx, float vy, float xo, float yo, int lane) {
    const int4 co = *reinterpret_cast<const int4 *>(coords + (size_t)p * 4);
    PfnPillar r;
    r.cx = __fadd_rn(__fmul_rn((float)co.w, vx), xo);
    r.cy = __fadd_rn(__fmul_rn((float)co.z, vy), yo);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    float zlo = INFINITY, zhi = -INFINITY;
    for (int t0 = 0; t0 < T; t0 += 64) {
        float4 q = (t0 + lane < T) ? pv[t0 + lane] : make_float4(0, 0, 0, 0);
        sx += q.x; sy += q.y; sz += q.z;
        if constexpr (KIND == kPfnRadiusHeight)
            if (t0 + lane < T) { zlo = fminf(zlo, q.z); zhi = fmaxf(zhi, q.z); }
    }
    const float inv = (float)n;
    r.mx = wave_sum(sx) / inv; r.my = wave_sum(sy) / inv; r.mz = wave_sum(sz) / inv;
    r.h = 0.f;
    if constexpr (KIND == kPfnRadiusHeight) r.h = wave_span(zlo, zhi);
    r.n = n < T ? n : T;
    return r;
}
template <int KIND, bool DIST>
__device__ __forceinline__ void pfn_decorate(const float4 q, const PfnPillar &pl, float (&f)[pfn_width(KIND, DIST)]) {
    pfn_row<KIND, DIST>(q, pl.mx, pl.my, pl.mz, pl.cx, pl.cy, pl.h, f);
}

// partial[block][c][StatVals], partial_s1[block][K], partial_d[block][c][2]; C <= 64 (one wave = all channels)
// sum x and sum x^2 are accumulated and handed on in fp64 (partial_d; slots 0 and 1 of `partial` stay unused): the variance is
// sum x^2 / N - mean^2, and a channel with |mean| >> std (a cloud offset from the origin, an intensity in 0..255) cancels there: at
// mean^2 / var = 550 fp32 sums per wave lost 3.8e-6 of invstd where torch's float32 BatchNorm keeps 2.2e-7 (the offset case of
// tests/test_gpu_pfn_edges.py); in fp64 the kernels keep 7e-8.
template <int KIND, bool DIST>
__global__ __launch_bounds__(kBlock) void k_pfn_stats(const float *__restrict__ voxels, const int *__restrict__ num_points,
                                                     const int *__restrict__ coords, int P, const int *__restrict__ num_dev, int T,
                                                     const float *__restrict__ wt, int C, float vx, float vy, float xo, float yo,
                                                     float *__restrict__ partial, float *__restrict__ partial_s1,
                                                     double *__restrict__ partial_d) {
    constexpr int K = PfnDims<KIND, DIST>::K, StatVals = PfnDims<KIND, DIST>::StatVals;
    P = pfn_live(num_dev, P);
    __shared__ float red[kBlock / 64][64][StatVals + 1];
    __shared__ float red1[kBlock / 64][K];
    __shared__ double redd[kBlock / 64][64][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool live = lane < C;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = live ? wt[(size_t)j * C + lane] : 0.f;
    float acc[StatVals], s1[K];
#pragma unroll
    for (int j = 0; j < StatVals; ++j) acc[j] = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) s1[j] = 0.f;
    double sum = 0.0, sq = 0.0;
    for (int p = blockIdx.x * (kBlock / 64) + wv; p < P; p += gridDim.x * (kBlock / 64)) {
        const float4 *pv = reinterpret_cast<const float4 *>(voxels) + (size_t)p * T;
        const PfnPillar pl = pfn_pillar<KIND>(pv, T, num_points[p], coords, p, vx, vy, xo, yo, lane);
        for (int t = 0; t < pl.n; ++t) {
            float f[K];
            pfn_decorate<KIND, DIST>(pv[t], pl, f);
            float x = 0.f;
#pragma unroll
            for (int j = 0; j < K; ++j) x = fmaf(f[j], w[j], x);
            sum += (double)x;
            sq = fma((double)x, (double)x, sq);
#pragma unroll
            for (int j = 0; j < K; ++j) { acc[2 + j] = fmaf(x, f[j], acc[2 + j]); s1[j] += f[j]; }
        }
    }
#pragma unroll
    for (int j = 0; j < StatVals; ++j) red[wv][lane][j] = acc[j];
    redd[wv][lane][0] = sum; redd[wv][lane][1] = sq;
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < K; ++j) red1[wv][j] = s1[j];
    __syncthreads();
    if (wv == 0) {
        if (live) {
#pragma unroll
            for (int j = 0; j < StatVals; ++j) {
                float v = 0.f;
                for (int k = 0; k < kBlock / 64; ++k) v += red[k][lane][j];
                partial[((size_t)blockIdx.x * C + lane) * StatVals + j] = v;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double v = 0.0;
                for (int k = 0; k < kBlock / 64; ++k) v += redd[k][lane][j];
                partial_d[((size_t)blockIdx.x * C + lane) * 2 + j] = v;
            }
        }
        if (lane < K) {
            float v = 0.f;
            for (int k = 0; k < kBlock / 64; ++k) v += red1[k][lane];
            partial_s1[(size_t)blockIdx.x * K + lane] = v;
        }
    }
}

__device__ __forceinline__ double block_sum_f64(double v, double *sh) {   // 256 threads
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int k = 0; k < kBlock / 64; ++k) r += sh[k];
    __syncthreads();
    return r;
}

// one block per channel (+ one for S1).  stats[c] layout: mean[C], invstd[C], M[C][K], S1[K]
template <int KIND, bool DIST>
__global__ __launch_bounds__(kBlock) void k_pfn_finalize(const float *__restrict__ partial, const float *__restrict__ partial_s1,
                                                        const double *__restrict__ partial_d, int blocks, int C, int P,
                                                        const int *__restrict__ num_dev, int T, float eps, float momentum,
                                                        float *__restrict__ running_mean, float *__restrict__ running_var,
                                                        float *__restrict__ stats) {
    constexpr int K = PfnDims<KIND, DIST>::K, StatVals = PfnDims<KIND, DIST>::StatVals;
    const double rows = (double)pfn_live(num_dev, P) * (double)T;      // BatchNorm's N: the live pillars' slots
    __shared__ double sh[kBlock / 64];
    const int c = blockIdx.x;
    if (c == C) {                                     // S1
        for (int j = 0; j < K; ++j) {
            double v = 0.0;
            for (int b = threadIdx.x; b < blocks; b += kBlock) v += (double)partial_s1[(size_t)b * K + j];
            v = block_sum_f64(v, sh);
            if (threadIdx.x == 0) stats[(size_t)C * (2 + K) + j] = (float)v;
        }
        return;
    }
    double tot[StatVals];
    for (int j = 0; j < StatVals; ++j) {
        double v = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kBlock)
            v += j < 2 ? partial_d[((size_t)b * C + c) * 2 + j] : (double)partial[((size_t)b * C + c) * StatVals + j];
        tot[j] = block_sum_f64(v, sh);
    }
    if (threadIdx.x == 0) {
        // no live pillar (rows == 0, every sum is zero): mean 0, variance 0, the running statistics keep their values
        const double mean = rows > 0.0 ? tot[0] / rows : 0.0;
        double var = rows > 0.0 ? tot[1] / rows - mean * mean : 0.0;
        if (var < 0.0) var = 0.0;
        stats[c] = (float)mean;
        stats[C + c] = (float)(1.0 / sqrt(var + (double)eps));
        for (int j = 0; j < K; ++j) stats[(size_t)2 * C + (size_t)c * K + j] = (float)tot[2 + j];
        if (rows > 0.0 && running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
        if (rows > 0.0 && running_var) running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * var * (rows > 1.0 ? rows / (rows - 1.0) : 1.0));
    }
}

// normalise with the batch statistics, ReLU, max over the slots; argmax[p][c] = slot of the maximum (first one; -1 = a padded slot)
template <int KIND, bool DIST>
__global__ __launch_bounds__(kBlock) void k_pfn_fwd_train(const float *__restrict__ voxels, const int *__restrict__ num_points,
                                                         const int *__restrict__ coords, int P, const int *__restrict__ num_dev, int T,
                                                         const float *__restrict__ wt,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta,
                                                         const float *__restrict__ stats, int C, float vx, float vy, float xo,
                                                         float yo, float *__restrict__ out, signed char *__restrict__ argmax) {
    constexpr int K = PfnDims<KIND, DIST>::K;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (p >= P) return;
    const bool live = lane < C;
    if (p >= pfn_live(num_dev, P)) {                  // a row of the capacity past the count: defined, and nothing of it is read
        if (live) {
            out[(size_t)p * C + lane] = 0.f;
            argmax[(size_t)p * C + lane] = (signed char)-1;
        }
        return;
    }
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = live ? wt[(size_t)j * C + lane] : 0.f;
    const float mean = live ? stats[lane] : 0.f, invstd = live ? stats[C + lane] : 0.f;
    const float ga = live ? gamma[lane] : 0.f, be = live ? beta[lane] : 0.f;
    const float4 *pv = reinterpret_cast<const float4 *>(voxels) + (size_t)p * T;
    const PfnPillar pl = pfn_pillar<KIND>(pv, T, num_points[p], coords, p, vx, vy, xo, yo, lane);
    float best = -INFINITY;
    int arg = -1;
    for (int t = 0; t < pl.n; ++t) {
        float f[K];
        pfn_decorate<KIND, DIST>(pv[t], pl, f);
        float x = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) x = fmaf(f[j], w[j], x);
        const float y = fmaxf(fmaf((x - mean) * invstd, ga, be), 0.f);
        if (y > best) { best = y; arg = t; }
    }
    if (pl.n < T) {                                   // padded slots: x = 0
        const float y = fmaxf(fmaf((0.f - mean) * invstd, ga, be), 0.f);
        if (y > best) { best = y; arg = -1; }
    }
    // statistics poisoned by a non-finite input (NaN mean or invstd): fmaxf and `y > best` drop the NaN that torch's relu and max
    // carry, so it is handed on here -- every output of the channel is NaN, as the reference's is
    if (mean != mean || invstd != invstd) best = __builtin_nanf("");
    if (live) {
        out[(size_t)p * C + lane] = best;
        argmax[(size_t)p * C + lane] = (signed char)arg;
    }
}

// partial[block][c][BwdVals] = (dbeta, dgamma, A[c][0..K-1])
template <int KIND, bool DIST>
__global__ __launch_bounds__(kBlock) void k_pfn_bwd(const float *__restrict__ voxels, const int *__restrict__ num_points,
                                                   const int *__restrict__ coords, int P, const int *__restrict__ num_dev, int T,
                                                   const float *__restrict__ wt, const float *__restrict__ stats, int C, float vx,
                                                   float vy, float xo, float yo,
                                                   const float *__restrict__ grad_out, const float *__restrict__ out,
                                                   const signed char *__restrict__ argmax, float *__restrict__ partial) {
    constexpr int K = PfnDims<KIND, DIST>::K, BwdVals = PfnDims<KIND, DIST>::BwdVals;
    P = pfn_live(num_dev, P);
    __shared__ float red[kBlock / 64][64][BwdVals + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool live = lane < C;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = live ? wt[(size_t)j * C + lane] : 0.f;
    const float mean = live ? stats[lane] : 0.f, invstd = live ? stats[C + lane] : 0.f;
    float acc[BwdVals];
#pragma unroll
    for (int j = 0; j < BwdVals; ++j) acc[j] = 0.f;
    for (int p = blockIdx.x * (kBlock / 64) + wv; p < P; p += gridDim.x * (kBlock / 64)) {
        const float4 *pv = reinterpret_cast<const float4 *>(voxels) + (size_t)p * T;
        const PfnPillar pl = pfn_pillar<KIND>(pv, T, num_points[p], coords, p, vx, vy, xo, yo, lane);
        if (!live) continue;
        const float g = grad_out[(size_t)p * C + lane];
        const float dz = out[(size_t)p * C + lane] > 0.f ? g : 0.f;
        const int t = argmax[(size_t)p * C + lane];
        float x = 0.f;
        float f[K];
#pragma unroll
        for (int j = 0; j < K; ++j) f[j] = 0.f;
        if (t >= 0) {
            pfn_decorate<KIND, DIST>(pv[t], pl, f);
#pragma unroll
            for (int j = 0; j < K; ++j) x = fmaf(f[j], w[j], x);
        }
        acc[0] += dz;
        acc[1] = fmaf(dz, (x - mean) * invstd, acc[1]);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[2 + j] = fmaf(dz, f[j], acc[2 + j]);
    }
#pragma unroll
    for (int j = 0; j < BwdVals; ++j) red[wv][lane][j] = acc[j];
    __syncthreads();
    if (wv == 0 && live)
#pragma unroll
        for (int j = 0; j < BwdVals; ++j) {
            float v = 0.f;
            for (int k = 0; k < kBlock / 64; ++k) v += red[k][lane][j];
            partial[((size_t)blockIdx.x * C + lane) * BwdVals + j] = v;
        }
}

// one block per channel: dweight_t[j][c], dgamma[c], dbeta[c]
template <int KIND, bool DIST>
__global__ __launch_bounds__(kBlock) void k_pfn_bwd_finalize(const float *__restrict__ partial, int blocks, int C, int P,
                                                            const int *__restrict__ num_dev, int T,
                                                            const float *__restrict__ gamma, const float *__restrict__ stats,
                                                            float *__restrict__ dweight_t, float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta) {
    constexpr int K = PfnDims<KIND, DIST>::K, BwdVals = PfnDims<KIND, DIST>::BwdVals;
    __shared__ double sh[kBlock / 64];
    const double rows = (double)pfn_live(num_dev, P) * (double)T;
    const int c = blockIdx.x;
    double tot[BwdVals];
    for (int j = 0; j < BwdVals; ++j) {
        double v = 0.0;
        for (int b = threadIdx.x; b < blocks; b += kBlock) v += (double)partial[((size_t)b * C + c) * BwdVals + j];
        tot[j] = block_sum_f64(v, sh);
    }
    if (threadIdx.x == 0) {
        const double mean = stats[c], invstd = stats[C + c], ga = gamma[c];
        const double db = tot[0], dg = tot[1];
        dbeta[c] = (float)db;
        dgamma[c] = (float)dg;
        for (int j = 0; j < K; ++j) {
            const double s1 = stats[(size_t)C * (2 + K) + j], m = stats[(size_t)2 * C + (size_t)c * K + j];
            // no live pillar: every sum is zero and so is the gradient (0 / 0 is not evaluated)
            dweight_t[(size_t)j * C + c] =
                rows > 0.0 ? (float)(ga * invstd * (tot[2 + j] - db / rows * s1 - dg / rows * invstd * (m - mean * s1))) : 0.f;
        }
    }
}

static int pfn_blocks(int P) {
    int b = div_up(P > 0 ? P : 1, kBlock / 64);
    return b > kPfnMaxBlocks ? kPfnMaxBlocks : b;
}

// ---- block filter ---------------------------------------------------------------------------------
__device__ __forceinline__ int f2ord(float f) {  // monotonic float -> int map for atomicMin/Max
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

struct BfParams {
    int T, F, batch, bx, by, block_factor, block_size;
    float thr, high;
};

__global__ __launch_bounds__(kBlock) void k_bf_init(int *__restrict__ mins, int *__restrict__ maxs, long long n) {
    long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n) return;
    mins[g] = f2ord(99999999.0f);
    maxs[g] = f2ord(-99999999.0f);
}

__global__ __launch_bounds__(kBlock) void k_bf_minmax(const float *__restrict__ voxels, const int *__restrict__ coors,
                                                     const int *__restrict__ num_points, const int *__restrict__ voff,
                                                     BfParams p, int *__restrict__ mins, int *__restrict__ maxs) {
    long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    int v = (int)(g / p.T), t = (int)(g % p.T);
    if (v >= voff[p.batch] || t >= num_points[v]) return;
    int4 c = *reinterpret_cast<const int4 *>(coors + (size_t)v * 4);
    int cell = (c.x * p.by + c.z / p.block_factor) * p.bx + c.w / p.block_factor;
    float z = voxels[((size_t)v * p.T + t) * p.F + 2];
    atomicMin(&mins[cell], f2ord(z));
    atomicMax(&maxs[cell], f2ord(z));
}

// The height-span test with one WAVE per voxel: lane l takes cell l of the (block_size x block_size <= 64-cell) window, the wave
// reduces min / max with shuffles.  (One thread per voxel walks its 64 cells x 2 arrays itself -- 128 loads on one thread's
// dependency chain: 214 us for the 360 k voxels of a nuscenes/all.fhd batch.)
__global__ __launch_bounds__(kBlock) void k_bf_mask_wave(const int *__restrict__ coors, const int *__restrict__ voff, BfParams p,
                                                        const int *__restrict__ mins, const int *__restrict__ maxs, int rows,
                                                        int *__restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= rows) return;
    if (v >= voff[p.batch]) { if (lane == 0) keep[v] = 0; return; }
    const int4 c = *reinterpret_cast<const int4 *>(coors + (size_t)v * 4);
    const int cy = c.z / p.block_factor, cx = c.w / p.block_factor;
    const int y0 = max(cy - p.block_size / 2, 0), y1 = min(cy + p.block_size - p.block_size / 2, p.by);
    const int x0 = max(cx - p.block_size / 2, 0), x1 = min(cx + p.block_size - p.block_size / 2, p.bx);
    float hmin = 99999999.0f, hmax = -99999999.0f;
    const int wx = x1 - x0, cells = wx * (y1 - y0);
    for (int e = lane; e < cells; e += 64) {
        const int y = y0 + e / wx, x = x0 + e % wx;
        const int cell = (c.x * p.by + y) * p.bx + x;
        hmin = fminf(hmin, ord2f(mins[cell]));
        hmax = fmaxf(hmax, ord2f(maxs[cell]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        hmin = fminf(hmin, __shfl_xor(hmin, d, 64));
        hmax = fmaxf(hmax, __shfl_xor(hmax, d, 64));
    }
    if (lane == 0) {
        const float span = __fsub_rn(hmax, hmin);
        keep[v] = (span > p.thr && span < p.high) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_bf_compact(const float *__restrict__ voxels, const int *__restrict__ coors,
                                                      const int *__restrict__ num_points, const int *__restrict__ voff,
                                                      const int *__restrict__ keep, const int *__restrict__ pos,
                                                      const int *__restrict__ total, BfParams p, int rows,
                                                      float *__restrict__ ov, int *__restrict__ oc, int *__restrict__ on,
                                                      int *__restrict__ ooff) {
    long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    int per = p.T * p.F;
    int v = (int)(g / per), e = (int)(g % per);
    if (g <= p.batch) {  // new per-cloud offsets: kept voxels before the cloud's first voxel
        int o = voff[g];
        ooff[g] = o < rows ? pos[o] : *total;
    }
    if (v >= voff[p.batch] || !keep[v]) return;
    int d = pos[v];
    ov[(size_t)d * per + e] = voxels[(size_t)v * per + e];
    if (e < 4) oc[(size_t)d * 4 + e] = coors[(size_t)v * 4 + e];
    if (e == 0) on[d] = num_points[v];
}

struct BfWorkspace {
    int *mins, *maxs, *keep, *pos, *scan, *total;
    size_t bytes;
};
static BfWorkspace carve_bf(void *ws, size_t cap, int rows, int batch, int bx, int by) {
    BfWorkspace w;
    Arena a(ws, cap);
    size_t cells = (size_t)batch * bx * by;
    w.mins = a.take<int>(cells);
    w.maxs = a.take<int>(cells);
    w.keep = a.take<int>(rows > 0 ? rows : 1);
    w.pos = a.take<int>(rows > 0 ? rows : 1);
    w.scan = a.take<int>(scan_scratch_ints(rows));
    w.total = a.take<int>(1);
    w.bytes = align_up(a.used);
    return w;
}

}  // namespace sec

using namespace sec;

// ---- PillarFeatureNet, host side: one path from the nineteen entry points to the kernels -------------------------------------------
// pfn_by_kind names the <KIND, DIST> instantiation; pfn_fwd, pfn_fwd_slots, pfn_train_fwd and pfn_train_bwd validate once and
// enqueue; every public function below them is one forwarding statement.
SEC_API int sec_pfn_row_width(int kind, int with_distance) {
    if (kind < kPfnPlain || kind > kPfnRadiusHeight || (with_distance != 0 && with_distance != 1)) return 0;
    return pfn_width(kind, with_distance != 0);
}

template <int KIND, bool DIST> struct PfnRow {
    static constexpr int kind = KIND;
    static constexpr bool dist = DIST;
};
// f(PfnRow<KIND, DIST>{}) for the pair the caller named, SEC_E_INVALID for a pair that names no row
template <class F> static int pfn_by_kind(int kind, int with_distance, F &&f) {
    if (!sec_pfn_row_width(kind, with_distance)) return SEC_E_INVALID;
    switch (kind * 2 + with_distance) {
    case kPfnPlain * 2: return f(PfnRow<kPfnPlain, false>{});
    case kPfnPlain * 2 + 1: return f(PfnRow<kPfnPlain, true>{});
    case kPfnRadius * 2: return f(PfnRow<kPfnRadius, false>{});
    case kPfnRadius * 2 + 1: return f(PfnRow<kPfnRadius, true>{});
    case kPfnOld * 2: return f(PfnRow<kPfnOld, false>{});
    case kPfnOld * 2 + 1: return f(PfnRow<kPfnOld, true>{});
    case kPfnRadiusHeight * 2: return f(PfnRow<kPfnRadiusHeight, false>{});
    default: return f(PfnRow<kPfnRadiusHeight, true>{});
    }
}

// k_pfn_fwd in the output type asked for.  `src`: the [P, T, 4] pillar tensor, or with SLOTS the flat point array behind `slots`.
template <bool SLOTS, int KIND, bool DIST>
static int pfn_fwd_launch(const float *src, const int *num_points, const int *coords, int num_pillars, const int *num_dev,
                          int max_points, const float *weight_t, const float *scale, const float *shift, int channels, float vx,
                          float vy, float x_offset, float y_offset, void *out, int out_dtype, const int *slots, void *stream) {
    if (num_pillars == 0) return SEC_OK;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(div_up(num_pillars, kBlock / 64)), block(kBlock);
#define SEC_PFN(OT) hipLaunchKernelGGL((k_pfn_fwd<OT, SLOTS, KIND, DIST>), grid, block, 0, st, src, num_points, coords, num_pillars, num_dev, \
                                       max_points, weight_t, scale, shift, channels, vx, vy, x_offset, y_offset, (OT *)out, slots)
    if (out_dtype == SEC_F32) SEC_PFN(float);
    else if (out_dtype == SEC_BF16) SEC_PFN(__hip_bfloat16);
    else if (out_dtype == SEC_F16) SEC_PFN(__half);
    else return SEC_E_UNSUPPORTED;
#undef SEC_PFN
    return check_launch();
}

static int pfn_fwd(int kind, int with_distance, const float *voxels, const int *num_points, const int *coords, int num_pillars,
                   const int *num_dev, int max_points, int num_features, const float *weight_t, const float *scale,
                   const float *shift, int channels, float vx, float vy, float x_offset, float y_offset, void *out, int out_dtype,
                   void *stream) {
    return pfn_by_kind(kind, with_distance, [&](auto row) -> int {
        if (num_pillars < 0 || max_points <= 0 || channels <= 0 || !weight_t || !scale || !shift || !out) return SEC_E_INVALID;
        if (num_features != 4) return SEC_E_UNSUPPORTED;  // x, y, z + one extra (reflectance / dt): every shipped config
        return pfn_fwd_launch<false, decltype(row)::kind, decltype(row)::dist>(voxels, num_points, coords, num_pillars, num_dev, max_points,
                                                                               weight_t, scale, shift, channels, vx, vy, x_offset,
                                                                               y_offset, out, out_dtype, nullptr, stream);
    });
}

static int pfn_fwd_slots(int kind, int with_distance, const float *points, const void *vox_workspace, size_t vox_workspace_bytes,
                         int vox_num_points, int vox_batch, int vox_max_voxels, int max_points, int num_features,
                         const int *num_points_per_voxel, const int *coords, int num_pillars, const int *num_dev,
                         const float *weight_t, const float *scale, const float *shift, int channels, float vx, float vy,
                         float x_offset, float y_offset, void *out, int out_dtype, void *stream) {
    return pfn_by_kind(kind, with_distance, [&](auto row) -> int {
        if (num_pillars < 0 || max_points <= 0 || channels <= 0 || !points || !vox_workspace || !num_points_per_voxel || !coords ||
            !weight_t || !scale || !shift || !out)
            return SEC_E_INVALID;
        if (num_features != 4) return SEC_E_UNSUPPORTED;
        if ((reinterpret_cast<uintptr_t>(points) & 15) != 0) return SEC_E_UNSUPPORTED;      // float4 gathers
        const int *count, *slots;
        if (!vox_slots_of(vox_workspace, vox_workspace_bytes, vox_num_points, vox_batch, vox_max_voxels, max_points, &count, &slots))
            return SEC_E_WORKSPACE;
        return pfn_fwd_launch<true, decltype(row)::kind, decltype(row)::dist>(points, num_points_per_voxel, coords, num_pillars, num_dev,
                                                                              max_points, weight_t, scale, shift, channels, vx, vy,
                                                                              x_offset, y_offset, out, out_dtype, slots, stream);
    });
}

// the training workspace for rows of `width` entries: partial[blocks][C][2 + width], partial_s1[blocks][width], partial_d[blocks][C][2]
static size_t pfn_train_ws_bytes(int width, int num_pillars, int channels) {
    if (num_pillars < 0 || channels <= 0 || channels > 64) return 0;
    const size_t b = (size_t)pfn_blocks(num_pillars);
    return align_up(b * channels * (2 + width) * sizeof(float)) + align_up(b * width * sizeof(float)) +
           align_up(b * channels * 2 * sizeof(double));
}

// `before`: the call came through one of the training entry points older than sec_pfn_kind_*.  Their callers hold two answers of
// theirs, which the two functions below keep; nothing else tells the older symbols from the kind forms.
// (1) The row width a training workspace is sized and carved for.  sec_pfn_train_workspace_bytes takes no kind, so what its callers
// allocate is for nine entries, the radius row's eight included, and the older forms carve by it; the kind forms by the kind's own
// K.  Only the offsets of the three arrays move: the per-block partials inside them are pitched by K either way.
template <int KIND, bool DIST> static constexpr int pfn_train_ws_width(bool before) {
    return before ? kPfnIn : PfnDims<KIND, DIST>::K;
}
// (2) The status of max_points > 127 (the int8 argmax cannot name the slot).  The older forms list T <= 127 with their argument checks
// (SEC_E_INVALID); sec_pfn_kind_* document it with the shape limits (SEC_E_UNSUPPORTED) and answer it ahead of the other checks.
static int pfn_train_long_pillar_status(bool before) { return before ? SEC_E_INVALID : SEC_E_UNSUPPORTED; }

static int pfn_train_fwd(bool before, int kind, int with_distance, const float *voxels, const int *num_points, const int *coords,
                         int num_pillars, const int *num_dev, int max_points, int num_features, const float *weight_t,
                         const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                         int channels, float vx, float vy, float x_offset, float y_offset, float *out, signed char *argmax,
                         float *stats, void *workspace, size_t workspace_bytes, void *stream) {
    return pfn_by_kind(kind, with_distance, [&](auto row) -> int {
        constexpr int KIND = decltype(row)::kind;
        constexpr bool DIST = decltype(row)::dist;
        if (max_points > 127) return pfn_train_long_pillar_status(before);
        if (num_pillars < 0 || max_points <= 0 || channels <= 0 || !weight_t || !gamma || !beta || !out || !argmax || !stats)
            return SEC_E_INVALID;
        if (num_features != 4 || channels > 64) return SEC_E_UNSUPPORTED;
        const int width = pfn_train_ws_width<KIND, DIST>(before);
        if (!workspace || workspace_bytes < pfn_train_ws_bytes(width, num_pillars, channels)) return SEC_E_WORKSPACE;
        if (num_pillars == 0 && !num_dev) return SEC_OK;
        hipStream_t st = (hipStream_t)stream;
        const int blocks = pfn_blocks(num_pillars);      // grids by capacity; every kernel reads the count itself (pfn_live)
        float *partial = (float *)workspace;
        float *partial_s1 = (float *)((char *)workspace + align_up((size_t)blocks * channels * (2 + width) * sizeof(float)));
        double *partial_d = (double *)((char *)partial_s1 + align_up((size_t)blocks * width * sizeof(float)));
        hipLaunchKernelGGL((k_pfn_stats<KIND, DIST>), dim3(blocks), dim3(kBlock), 0, st, voxels, num_points, coords, num_pillars, num_dev,
                           max_points, weight_t, channels, vx, vy, x_offset, y_offset, partial, partial_s1, partial_d);
        hipLaunchKernelGGL((k_pfn_finalize<KIND, DIST>), dim3(channels + 1), dim3(kBlock), 0, st, partial, partial_s1, partial_d, blocks,
                           channels, num_pillars, num_dev, max_points, eps, momentum, running_mean, running_var, stats);
        if (num_pillars == 0) return check_launch();    // a capacity of zero: the statistics of no pillar, nothing else to write
        hipLaunchKernelGGL((k_pfn_fwd_train<KIND, DIST>), dim3(div_up(num_pillars, kBlock / 64)), dim3(kBlock), 0, st, voxels, num_points,
                           coords, num_pillars, num_dev, max_points, weight_t, gamma, beta, stats, channels, vx, vy, x_offset, y_offset, out,
                           argmax);
        return check_launch();
    });
}

static int pfn_train_bwd(bool before, int kind, int with_distance, const float *voxels, const int *num_points, const int *coords,
                         int num_pillars, const int *num_dev, int max_points, int num_features, const float *weight_t,
                         const float *gamma, const float *stats, int channels, float vx, float vy, float x_offset, float y_offset,
                         const float *grad_out, const float *out, const signed char *argmax, float *dweight_t, float *dgamma,
                         float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
    return pfn_by_kind(kind, with_distance, [&](auto row) -> int {
        constexpr int KIND = decltype(row)::kind;
        constexpr bool DIST = decltype(row)::dist;
        if (max_points > 127) return pfn_train_long_pillar_status(before);
        if (num_pillars < 0 || max_points <= 0 || channels <= 0 || !weight_t || !gamma || !stats || !grad_out || !out || !argmax ||
            !dweight_t || !dgamma || !dbeta)
            return SEC_E_INVALID;
        if (num_features != 4 || channels > 64) return SEC_E_UNSUPPORTED;
        if (!workspace || workspace_bytes < pfn_train_ws_bytes(pfn_train_ws_width<KIND, DIST>(before), num_pillars, channels))
            return SEC_E_WORKSPACE;
        hipStream_t st = (hipStream_t)stream;
        if (num_pillars == 0) {
            int rc = fill_words(dweight_t, sizeof(float) * PfnDims<KIND, DIST>::K * channels, 0u, st);
            if (!rc) rc = fill_words(dgamma, sizeof(float) * channels, 0u, st);
            if (!rc) rc = fill_words(dbeta, sizeof(float) * channels, 0u, st);
            return rc;
        }
        const int blocks = pfn_blocks(num_pillars);
        float *partial = (float *)workspace;
        hipLaunchKernelGGL((k_pfn_bwd<KIND, DIST>), dim3(blocks), dim3(kBlock), 0, st, voxels, num_points, coords, num_pillars, num_dev,
                           max_points, weight_t, stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, partial);
        hipLaunchKernelGGL((k_pfn_bwd_finalize<KIND, DIST>), dim3(channels), dim3(kBlock), 0, st, partial, blocks, channels, num_pillars,
                           num_dev, max_points, gamma, stats, dweight_t, dgamma, dbeta);
        return check_launch();
    });
}

// -- the public functions: (kind, with_distance) from the caller, or fixed by the symbol's name; num_dev from the caller (the _live
// forms: static capacity, the first min(max(*num_dev, 0), num_pillars) rows are pillars), or NULL: every row is a pillar
SEC_API int sec_pfn_kind_fwd(int kind, int with_distance, const float *voxels, const int *num_points, const int *coords,
                             int num_pillars, const int *num_dev, int max_points, int num_features, const float *weight_t,
                             const float *scale, const float *shift, int channels, float vx, float vy, float x_offset,
                             float y_offset, void *out, int out_dtype, void *stream) {
    return pfn_fwd(kind, with_distance, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, scale, shift,
                   channels, vx, vy, x_offset, y_offset, out, out_dtype, stream);
}
SEC_API int sec_pfn_fwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, const int *num_dev,
                        int max_points, int num_features, const float *weight_t, const float *scale, const float *shift,
                        int channels, float vx, float vy, float x_offset, float y_offset, void *out, int out_dtype,
                        void *stream) {
    return pfn_fwd(kPfnPlain, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, scale, shift,
                   channels, vx, vy, x_offset, y_offset, out, out_dtype, stream);
}
// PillarFeatureNetRadius: the same arguments, weight_t is [num_features + 4][channels]
SEC_API int sec_pfn_radius_fwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, const int *num_dev,
                               int max_points, int num_features, const float *weight_t, const float *scale, const float *shift,
                               int channels, float vx, float vy, float x_offset, float y_offset, void *out, int out_dtype,
                               void *stream) {
    return pfn_fwd(kPfnRadius, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, scale, shift,
                   channels, vx, vy, x_offset, y_offset, out, out_dtype, stream);
}

SEC_API int sec_pfn_kind_fwd_slots(int kind, int with_distance, const float *points, const void *vox_workspace,
                                   size_t vox_workspace_bytes, int vox_num_points, int vox_batch, int vox_max_voxels, int max_points,
                                   int num_features, const int *num_points_per_voxel, const int *coords, int num_pillars,
                                   const int *num_dev, const float *weight_t, const float *scale, const float *shift, int channels,
                                   float vx, float vy, float x_offset, float y_offset, void *out, int out_dtype, void *stream) {
    return pfn_fwd_slots(kind, with_distance, points, vox_workspace, vox_workspace_bytes, vox_num_points, vox_batch, vox_max_voxels,
                         max_points, num_features, num_points_per_voxel, coords, num_pillars, num_dev, weight_t, scale, shift, channels,
                         vx, vy, x_offset, y_offset, out, out_dtype, stream);
}
SEC_API int sec_pfn_fwd_slots(const float *points, const void *vox_workspace, size_t vox_workspace_bytes, int vox_num_points,
                              int vox_batch, int vox_max_voxels, int max_points, int num_features, const int *num_points_per_voxel,
                              const int *coords, int num_pillars, const int *num_dev, const float *weight_t, const float *scale,
                              const float *shift, int channels, float vx, float vy, float x_offset, float y_offset, void *out,
                              int out_dtype, void *stream) {
    return pfn_fwd_slots(kPfnPlain, 0, points, vox_workspace, vox_workspace_bytes, vox_num_points, vox_batch, vox_max_voxels,
                         max_points, num_features, num_points_per_voxel, coords, num_pillars, num_dev, weight_t, scale, shift, channels,
                         vx, vy, x_offset, y_offset, out, out_dtype, stream);
}
SEC_API int sec_pfn_radius_fwd_slots(const float *points, const void *vox_workspace, size_t vox_workspace_bytes, int vox_num_points,
                                     int vox_batch, int vox_max_voxels, int max_points, int num_features,
                                     const int *num_points_per_voxel, const int *coords, int num_pillars, const int *num_dev,
                                     const float *weight_t, const float *scale, const float *shift, int channels, float vx, float vy,
                                     float x_offset, float y_offset, void *out, int out_dtype, void *stream) {
    return pfn_fwd_slots(kPfnRadius, 0, points, vox_workspace, vox_workspace_bytes, vox_num_points, vox_batch, vox_max_voxels,
                         max_points, num_features, num_points_per_voxel, coords, num_pillars, num_dev, weight_t, scale, shift, channels,
                         vx, vy, x_offset, y_offset, out, out_dtype, stream);
}

SEC_API size_t sec_pfn_kind_train_workspace_bytes(int kind, int with_distance, int num_pillars, int channels) {
    size_t bytes = 0;      // stays zero for a pair that names no row
    pfn_by_kind(kind, with_distance, [&](auto row) -> int {
        bytes = pfn_train_ws_bytes(pfn_train_ws_width<decltype(row)::kind, decltype(row)::dist>(false), num_pillars, channels);
        return SEC_OK;
    });
    return bytes;
}
SEC_API size_t sec_pfn_train_workspace_bytes(int num_pillars, int channels) {
    return pfn_train_ws_bytes(pfn_train_ws_width<kPfnPlain, false>(true), num_pillars, channels);
}

SEC_API int sec_pfn_kind_train_fwd(int kind, int with_distance, const float *voxels, const int *num_points, const int *coords,
                                   int num_pillars, const int *num_dev, int max_points, int num_features, const float *weight_t,
                                   const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                                   float *running_var, int channels, float vx, float vy, float x_offset, float y_offset, float *out,
                                   signed char *argmax, float *stats, void *workspace, size_t workspace_bytes, void *stream) {
    return pfn_train_fwd(false, kind, with_distance, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t,
                         gamma, beta, eps, momentum, running_mean, running_var, channels, vx, vy, x_offset, y_offset, out, argmax, stats,
                         workspace, workspace_bytes, stream);
}
SEC_API int sec_pfn_train_fwd_live(const float *voxels, const int *num_points, const int *coords, int num_pillars, const int *num_dev,
                                   int max_points, int num_features, const float *weight_t, const float *gamma, const float *beta,
                                   float eps, float momentum, float *running_mean, float *running_var, int channels, float vx,
                                   float vy, float x_offset, float y_offset, float *out, signed char *argmax, float *stats,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    return pfn_train_fwd(true, kPfnPlain, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, gamma,
                         beta, eps, momentum, running_mean, running_var, channels, vx, vy, x_offset, y_offset, out, argmax, stats,
                         workspace, workspace_bytes, stream);
}
// PillarFeatureNetRadius in training mode: the same arguments, weight_t / dweight_t are [8][channels]
SEC_API int sec_pfn_radius_train_fwd_live(const float *voxels, const int *num_points, const int *coords, int num_pillars,
                                          const int *num_dev, int max_points, int num_features, const float *weight_t,
                                          const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                                          float *running_var, int channels, float vx, float vy, float x_offset, float y_offset,
                                          float *out, signed char *argmax, float *stats, void *workspace, size_t workspace_bytes,
                                          void *stream) {
    return pfn_train_fwd(true, kPfnRadius, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, gamma,
                         beta, eps, momentum, running_mean, running_var, channels, vx, vy, x_offset, y_offset, out, argmax, stats,
                         workspace, workspace_bytes, stream);
}
SEC_API int sec_pfn_train_fwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, int max_points,
                              int num_features, const float *weight_t, const float *gamma, const float *beta, float eps,
                              float momentum, float *running_mean, float *running_var, int channels, float vx, float vy,
                              float x_offset, float y_offset, float *out, signed char *argmax, float *stats, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return pfn_train_fwd(true, kPfnPlain, 0, voxels, num_points, coords, num_pillars, nullptr, max_points, num_features, weight_t, gamma,
                         beta, eps, momentum, running_mean, running_var, channels, vx, vy, x_offset, y_offset, out, argmax, stats,
                         workspace, workspace_bytes, stream);
}
SEC_API int sec_pfn_radius_train_fwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, int max_points,
                                     int num_features, const float *weight_t, const float *gamma, const float *beta, float eps,
                                     float momentum, float *running_mean, float *running_var, int channels, float vx, float vy,
                                     float x_offset, float y_offset, float *out, signed char *argmax, float *stats, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return pfn_train_fwd(true, kPfnRadius, 0, voxels, num_points, coords, num_pillars, nullptr, max_points, num_features, weight_t, gamma,
                         beta, eps, momentum, running_mean, running_var, channels, vx, vy, x_offset, y_offset, out, argmax, stats,
                         workspace, workspace_bytes, stream);
}

SEC_API int sec_pfn_kind_train_bwd(int kind, int with_distance, const float *voxels, const int *num_points, const int *coords,
                                   int num_pillars, const int *num_dev, int max_points, int num_features, const float *weight_t,
                                   const float *gamma, const float *stats, int channels, float vx, float vy, float x_offset,
                                   float y_offset, const float *grad_out, const float *out, const signed char *argmax,
                                   float *dweight_t, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    return pfn_train_bwd(false, kind, with_distance, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t,
                         gamma, stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, dweight_t, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}
SEC_API int sec_pfn_train_bwd_live(const float *voxels, const int *num_points, const int *coords, int num_pillars, const int *num_dev,
                                   int max_points, int num_features, const float *weight_t, const float *gamma, const float *stats,
                                   int channels, float vx, float vy, float x_offset, float y_offset, const float *grad_out,
                                   const float *out, const signed char *argmax, float *dweight_t, float *dgamma, float *dbeta,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    return pfn_train_bwd(true, kPfnPlain, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, gamma,
                         stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, dweight_t, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}
SEC_API int sec_pfn_radius_train_bwd_live(const float *voxels, const int *num_points, const int *coords, int num_pillars,
                                          const int *num_dev, int max_points, int num_features, const float *weight_t,
                                          const float *gamma, const float *stats, int channels, float vx, float vy, float x_offset,
                                          float y_offset, const float *grad_out, const float *out, const signed char *argmax,
                                          float *dweight_t, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                          void *stream) {
    return pfn_train_bwd(true, kPfnRadius, 0, voxels, num_points, coords, num_pillars, num_dev, max_points, num_features, weight_t, gamma,
                         stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, dweight_t, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}
SEC_API int sec_pfn_train_bwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, int max_points,
                              int num_features, const float *weight_t, const float *gamma, const float *stats, int channels, float vx,
                              float vy, float x_offset, float y_offset, const float *grad_out, const float *out,
                              const signed char *argmax, float *dweight_t, float *dgamma, float *dbeta, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return pfn_train_bwd(true, kPfnPlain, 0, voxels, num_points, coords, num_pillars, nullptr, max_points, num_features, weight_t, gamma,
                         stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, dweight_t, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}
SEC_API int sec_pfn_radius_train_bwd(const float *voxels, const int *num_points, const int *coords, int num_pillars, int max_points,
                                     int num_features, const float *weight_t, const float *gamma, const float *stats, int channels,
                                     float vx, float vy, float x_offset, float y_offset, const float *grad_out, const float *out,
                                     const signed char *argmax, float *dweight_t, float *dgamma, float *dbeta, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return pfn_train_bwd(true, kPfnRadius, 0, voxels, num_points, coords, num_pillars, nullptr, max_points, num_features, weight_t, gamma,
                         stats, channels, vx, vy, x_offset, y_offset, grad_out, out, argmax, dweight_t, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}

SEC_API size_t sec_block_filter_workspace_bytes(int rows, int batch, int grid_x, int grid_y, int block_factor) {
    if (rows < 0 || batch <= 0 || block_factor <= 0) return 0;
    return carve_bf(nullptr, 0, rows, batch, div_up(grid_x, block_factor), div_up(grid_y, block_factor)).bytes;
}

SEC_API int sec_voxel_block_filter_f32(const float *voxels, const int *coors, const int *num_points,
                                       const int *voxel_offsets, int rows, int batch, int max_points, int num_features,
                                       int grid_x, int grid_y, int block_factor, int block_size, float height_threshold,
                                       float height_high_threshold, float *out_voxels, int *out_coors,
                                       int *out_num_points, int *out_offsets, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    if (rows < 0 || batch <= 0 || max_points <= 0 || num_features < 3 || block_factor <= 0 || block_size <= 0 ||
        !voxel_offsets || !out_offsets)
        return SEC_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    BfParams p{max_points, num_features, batch, div_up(grid_x, block_factor), div_up(grid_y, block_factor), block_factor,
               block_size, height_threshold, height_high_threshold};
    BfWorkspace w = carve_bf(workspace, workspace_bytes, rows, batch, p.bx, p.by);
    if (!workspace || w.bytes > workspace_bytes) return SEC_E_WORKSPACE;
    long long cells = (long long)batch * p.bx * p.by;
    hipLaunchKernelGGL(k_bf_init, dim3(div_up(cells, kBlock)), dim3(kBlock), 0, st, w.mins, w.maxs, cells);
    int rc;
    if (rows > 0) {
        hipLaunchKernelGGL(k_bf_minmax, dim3(div_up((long long)rows * max_points, kBlock)), dim3(kBlock), 0, st, voxels,
                           coors, num_points, voxel_offsets, p, w.mins, w.maxs);
        hipLaunchKernelGGL(k_bf_mask_wave, dim3(div_up(rows, kBlock / 64)), dim3(kBlock), 0, st, coors, voxel_offsets, p, w.mins,
                           w.maxs, rows, w.keep);
    }
    if ((rc = exclusive_scan_i32(w.keep, w.pos, rows, w.total, w.scan, st))) return rc;
    long long work = (long long)(rows > 0 ? rows : 1) * max_points * num_features;
    if (work < batch + 1) work = batch + 1;
    hipLaunchKernelGGL(k_bf_compact, dim3(div_up(work, kBlock)), dim3(kBlock), 0, st, voxels, coors, num_points,
                       voxel_offsets, w.keep, w.pos, w.total, p, rows, out_voxels, out_coors, out_num_points, out_offsets);
    return check_launch();
}
