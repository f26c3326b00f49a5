// Device-resident post-processing of VoxelNet.predict (second/pytorch/models/voxelnet.py:377-645):
//   sec_predict_select   : best class per anchor, score threshold, top-k by score, sorted descending
//                          (torch.sigmoid / max / masked_select / topk of voxelnet.py:545-569 and
//                          box_torch_ops.py:497-501) -- one workgroup per frame: 8-bit radix select over
//                          order-preserving keys, ordered tie handling, bitonic sort of the k survivors in LDS;
//   sec_predict_decode   : gather + second_box_decode (box_torch_ops.py:56-101) of the selected anchors, NMS input
//                          rows (rotated (x,y,w,l,r,score) or standup (x1,y1,x2,y2,score)), direction argmax;
//   sec_predict_finalize : gather of the NMS survivors, direction fix (limit_period, voxelnet.py:598-607),
//                          post_center_range mask (:611-621);
//   sec_predict_select_classes / _decode_classes / _finalize_classes : the same chain for use_multi_class_nms (voxelnet.py:458-547)
//                          with (frame, class) items as the unit of work (per-class anchor range, column, threshold, k, post_max).
// The reference runs ~60 tiny torch kernels plus a GPU->CPU->GPU round trip here; these three launches plus the
// two NMS launches keep everything on the device with fixed shapes (hipGraph friendly).
// Tensors are addressed as logit(b, anchor n = (a, y, x), c) = base[b*sb + a*sa + y*sy + x*sx + c*sc] so the RPN head
// output is consumed in place (no permute / contiguous copies).
#include "common.hpp"
#include <type_traits>

namespace sec {

struct View5 {          // element strides of a [B, A, H, W, C] view
    long long sb, sa, sy, sx, sc;
    // LAZY heads (sec_predict_select_lazy / _decode_lazy): the producer (sec_conv1x1_chain_nhwc_tiles with background == NULL) wrote
    // only the tiles its live list names.  `live` [B][tiles] (8 x 16 tiles, row-major) holds bit 4 = "this tile was written"; for
    // every other tile the element is read from the empty frame's head map instead -- `bg` = its element offset relative to the
    // view's base pointer (same sa / sy / sx / sc, no frame stride): exactly the value the producer's copy would have put there.
    long long bg;
    const unsigned short *live;
    int tiles_x, tpf;
    // anchor-area mask (sec_predict_select_masked): amask[b * A*H*W + n] == 0 takes anchor n of frame b out of the selection -- its key
    // is the smallest one (0: below every logit's, the key of the slots past a frame's end), whose score never reaches a threshold > 0
    const unsigned char *amask;
    // COVER form of the lazy heads (sec_predict_select_cover / _decode_cover): the producer's tiles start at any column of their 8-row
    // band (sec_rpn_tile_cover), so "written" is a bit per pixel column and band: `cover` [B][bands][cwr] words, bit x & 31 of word x >> 5
    const unsigned *cover;
    int cwr, cbands;
};
__device__ __forceinline__ bool anchor_kept(const View5 &v, long long slot) { return !v.amask || v.amask[slot] != 0; }
// element offset of frame b as seen from pixel (y, x): the frame itself, or the empty frame's map for a tile that was never written
__device__ __forceinline__ long long frame_off(const View5 &v, int b, int y, int x) {
    if (v.cover) {
        const unsigned m = v.cover[((long long)b * v.cbands + (y >> 3)) * v.cwr + (x >> 5)];
        if (!((m >> (x & 31)) & 1u)) return v.bg;
    } else if (v.live) {
        const unsigned m = v.live[(long long)b * v.tpf + (y >> 3) * v.tiles_x + (x >> 4)];
        if (!((m >> 4) & 1u)) return v.bg;
    }
    return (long long)b * v.sb;
}
struct PredGeom {
    int batch, A, H, W, nc;   // anchors per location, feature map, classes
};

template <typename T> __device__ __forceinline__ float ldf(const T *p);
template <> __device__ __forceinline__ float ldf(const float *p) { return *p; }
template <> __device__ __forceinline__ float ldf(const __hip_bfloat16 *p) { return __bfloat162float(*p); }
template <> __device__ __forceinline__ float ldf(const __half *p) { return __half2float(*p); }

__device__ __forceinline__ unsigned f2key(float f) {   // order-preserving float -> uint
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// 16-bit order-preserving keys of 16-bit logits.  bf16: the high half of f2key(float(x)) (a bf16 is the high half of its float);
// fp16: the same sign trick on the half's own bits (all 16 bits are significant, none are lost).  key16_score() is the sigmoid of
// the logit a key stands for.
template <typename T> __device__ __forceinline__ unsigned key16_of(float best);
template <> __device__ __forceinline__ unsigned key16_of<__hip_bfloat16>(float best) { return f2key(best) >> 16; }
template <> __device__ __forceinline__ unsigned key16_of<__half>(float best) {
    const unsigned u = __half_as_ushort(__float2half_rn(best));      // exact: `best` came from a half
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}
template <> __device__ __forceinline__ unsigned key16_of<float>(float best) { return f2key(best) >> 16; }   // unused (fp32 heads take the 32-bit path)
template <typename T> __device__ __forceinline__ float key16_logit(unsigned k);
template <> __device__ __forceinline__ float key16_logit<__hip_bfloat16>(unsigned k) {
    return key2f((k << 16) | ((k & 0x8000u) ? 0u : 0xffffu));        // low half of f2key: 0 for a non-negative bf16, 0xffff for a negative one
}
template <> __device__ __forceinline__ float key16_logit<__half>(unsigned k) {
    const unsigned u = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    return __half2float(__ushort_as_half((unsigned short)u));
}
template <> __device__ __forceinline__ float key16_logit<float>(unsigned k) { return key16_logit<__hip_bfloat16>(k); }

template <typename T>
__device__ __forceinline__ unsigned anchor_key(const T *cls, const View5 &v, const PredGeom &g, int b, int n, int *label) {
    int x = n % g.W;
    int t = n / g.W;
    int y = t % g.H;
    int a = t / g.H;
    const T *p = cls + frame_off(v, b, y, x) + a * v.sa + y * v.sy + x * v.sx;
    float best = ldf(p);
    int lab = 0;
    for (int c = 1; c < g.nc; ++c) {
        float f = ldf(p + c * v.sc);
        if (f > best || f != f) { best = f; lab = c; }                 // NaN-propagating maximum (torch.max of voxelnet.py:558)
    }
    if (label) *label = lab;
    if (!anchor_kept(v, (long long)b * g.A * g.H * g.W + n) || best != best) return 0u;   // a NaN score reaches no threshold: key of a masked anchor
    return f2key(best);
}

// ---- several head tensors (sec_predict_select_segments / _decode_segments) ------------------------------------------------
// A multi-head network (nuscenes/all.pp.mhead: a 100 x 100 map with 12 anchors per cell next to a 160 x 160 map with 8) predicts
// into S tensors of different map size; target_assigner.generate_anchors concatenates their anchors class-major, so the global
// anchor n lies in the segment s with start[s] <= n < start[s + 1] and is that segment's anchor n - start[s] = (a * H_s + y) * W_s
// + x.  SegView stands where a View5 stands in the kernels below (template parameter V): keys, ranking and ties are by GLOBAL index
// and never see the segments; only the address of an anchor's logits does.  No lazy form, no anchor mask.
constexpr int kMaxSegments = 4;
struct Seg {
    const void *base;
    long long sb, sa, sy, sx, sc;
    int H, W;
    int start;                        // anchors before this segment; the total for an unused entry
};
struct SegView {                      // named members, no arrays: as a kernel argument it is read field by field, never copied to scratch
    Seg g0, g1, g2, g3;
    int total;
};
// The segment a thread currently walks: frame b's first element of it, its strides and map, and where its anchors end
template <typename T> struct SegCur {
    const T *frame;
    long long sa, sy, sx, sc;
    int H, W, end;
};
template <typename X> __device__ __forceinline__ X seg_pick(int s, X a, X b, X c, X d) {   // the s-th of four VALUES
    X r = a;
    r = s >= 1 ? b : r;
    r = s >= 2 ? c : r;
    r = s >= 3 ? d : r;
    return r;
}
// enter the segment of global anchor n (a chain of selects over the four named segments); (a, y, x) of n by division
template <typename T>
__device__ __forceinline__ void seg_enter(const SegView &v, int b, int n, SegCur<T> &c, int &x, int &y, int &a) {
    // every field is read from the kernel argument unconditionally and the segment's picked by value: conditional reads made the
    // compiler keep a per-lane copy of the table in scratch memory (232 bytes) and select between addresses into it
    const int s = (n >= v.g1.start ? 1 : 0) + (n >= v.g2.start ? 1 : 0) + (n >= v.g3.start ? 1 : 0);
#define SEC_SEG_PICK(F) seg_pick(s, v.g0.F, v.g1.F, v.g2.F, v.g3.F)
    const void *base = SEC_SEG_PICK(base);
    const long long sb = SEC_SEG_PICK(sb);
    const int first = SEC_SEG_PICK(start);
    c.sa = SEC_SEG_PICK(sa); c.sy = SEC_SEG_PICK(sy); c.sx = SEC_SEG_PICK(sx); c.sc = SEC_SEG_PICK(sc);
    c.H = SEC_SEG_PICK(H); c.W = SEC_SEG_PICK(W);
    c.end = seg_pick(s, v.g1.start, v.g2.start, v.g3.start, v.total);
#undef SEC_SEG_PICK
    static_assert(kMaxSegments == 4, "SegView names four segments");
    c.frame = static_cast<const T *>(base) + (long long)b * sb;
    const int l = n - first;
    x = l % c.W;
    const int t = l / c.W;
    y = t % c.H;
    a = t / c.H;
}
// the logits of global anchor n in frame b, and their channel stride
template <typename T> __device__ __forceinline__ const T *seg_anchor(const SegView &v, int b, int n, long long *sc) {
    SegCur<T> c;
    int x, y, a;
    seg_enter(v, b, n, c, x, y, a);
    *sc = c.sc;
    return c.frame + a * c.sa + y * c.sy + x * c.sx;
}
template <typename T>
__device__ __forceinline__ unsigned anchor_key(const T *, const SegView &v, const PredGeom &g, int b, int n, int *label) {
    long long sc;
    const T *p = seg_anchor<T>(v, b, n, &sc);
    float best = ldf(p);
    int lab = 0;
    for (int c = 1; c < g.nc; ++c) {
        float f = ldf(p + c * sc);
        if (f > best || f != f) { best = f; lab = c; }                 // as the View5 form: NaN propagates and takes key 0
    }
    if (label) *label = lab;
    return best != best ? 0u : f2key(best);
}

constexpr int kSelThreads = 1024;
constexpr int kCandCap = 2048;      // k_predict_select_reg: keys kept in LDS once that few remain above the bisection bound

// pass 0 (whole chip): compact, coalesced key array (the RPN head is channels-last: one anchor's logit per 128-byte
// pixel row, far too scattered to be re-read by the single workgroup that owns a frame in the select kernel)
template <typename T, typename V = View5>
__global__ __launch_bounds__(kBlock) void k_predict_keys(const T *__restrict__ cls, V v, PredGeom g,
                                                        unsigned *__restrict__ keys) {
    const int N = g.A * g.H * g.W;
    long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)g.batch * N) return;
    keys[t] = anchor_key(cls, v, g, (int)(t / N), (int)(t % N), nullptr);
}

// 16-bit form for 16-bit logits (the low half of such a key is implied by its sign bit): half the bytes, and two
// consecutive anchors' keys arrive in one dword load in k_predict_select_reg.  Frame stride `ns` is N rounded up to even.
template <typename T, typename V = View5>
__global__ __launch_bounds__(kBlock) void k_predict_keys16(const T *__restrict__ cls, V v, PredGeom g, int ns,
                                                          unsigned short *__restrict__ keys) {
    const int N = g.A * g.H * g.W;
    long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)g.batch * ns) return;
    const int b = (int)(t / ns), n = (int)(t % ns);
    const unsigned k32 = n < N ? anchor_key(cls, v, g, b, n, nullptr) : 0u;                  // 0: past the frame, or masked out
    keys[t] = k32 ? (unsigned short)key16_of<T>(key2f(k32)) : (unsigned short)0;
}

// one workgroup per frame
template <typename T, bool KEY16, typename V = View5>
__global__ __launch_bounds__(kSelThreads) void k_predict_select(const T *__restrict__ cls, V v, PredGeom g, int K,
                                                                float score_thr, const unsigned *__restrict__ keys,
                                                                int *__restrict__ top_idx,
                                                                float *__restrict__ top_score, int *__restrict__ top_label,
                                                                int *__restrict__ counts, unsigned thr_key = 0u) {
    __shared__ unsigned hist[256];
    __shared__ unsigned ckey[kSelThreads];
    __shared__ int cidx[kSelThreads];
    __shared__ int wsum[kSelThreads / 64];
    __shared__ unsigned s_prefix, s_need;
    __shared__ int s_cnt, s_eqbase;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = g.A * g.H * g.W;
    const unsigned *fk = keys + (size_t)b * N;
    if (K > kSelThreads) K = kSelThreads;
    if (K > N) K = N;
    // ---- radix select of the K-th largest key (8 bits per pass, MSB first).  bf16 logits only carry 16 key bits
    //      (the low half of the fp32 pattern is zero): two passes instead of four.
    constexpr int UNR = 8;                       // independent key loads in flight per thread
    const int first_shift = 24, last_shift = sizeof(T) == 2 && KEY16 ? 16 : 0;
    unsigned prefix = 0, mask = 0, need = K;
    // Threshold shortcut (round 5; the 16-bit paths have had it since round 3): `thr_key` is a key no larger than that of any logit
    // whose sigmoid reaches the score threshold.  A trained head leaves a few hundred such anchors per frame: when they are at most
    // K, they ARE the selection (rows behind counts[b] are unspecified by contract), and the four radix sweeps are skipped.
    bool shortcut = false;
    if (thr_key > 1u) {
        if (tid == 0) hist[0] = 0u;
        __syncthreads();
        unsigned c = 0;
        for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
            unsigned kk[UNR];
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                const int n = n0 + j * kSelThreads + tid;
                kk[j] = ld_sel(fk, n, n < N, 0u);
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) c += kk[j] >= thr_key ? 1u : 0u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0 && c) atomicAdd(&hist[0], c);
        __syncthreads();
        shortcut = hist[0] <= (unsigned)K;
        __syncthreads();
        if (shortcut) { prefix = thr_key - 1u; need = 0u; }
    }
    for (int shift = first_shift; !shortcut && shift >= last_shift; shift -= 8) {
        for (int i = tid; i < 256; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
            unsigned kk[UNR];
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                int n = n0 + j * kSelThreads + tid;
                kk[j] = ld_sel(fk, n, n < N, 0u);
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                int n = n0 + j * kSelThreads + tid;
                bool act = n < N && (kk[j] & mask) == prefix;
                unsigned d = (kk[j] >> shift) & 255u;
                if (shift == first_shift) {
                    // sign/exponent byte: a handful of distinct values -> wave-aggregated update (a uniform digit
                    // costs one LDS atomic per wave instead of a 64-way conflict)
                    unsigned long long todo = __ballot(act);
                    while (todo) {
                        int leader = __ffsll((long long)todo) - 1;
                        unsigned d0 = __shfl(d, leader, 64);
                        unsigned long long same = __ballot(act && d == d0) & todo;
                        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
                        todo &= ~same;
                    }
                } else if (act) {
                    atomicAdd(&hist[d], 1u);      // mantissa bytes are well spread and only the prefix matches are active
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned acc = 0;
            int bin = 255;
            for (; bin > 0; --bin) {
                if (acc + hist[bin] >= need) break;
                acc += hist[bin];
            }
            s_prefix = prefix | ((unsigned)bin << shift);
            s_need = need - acc;     // how many still to take inside this bin
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
        mask |= 255u << shift;
        __syncthreads();
    }
    // K-th largest key; take all keys > T and the first `need` (by index) equal to T.  The two KEY16 passes resolved the high half
    // only: the low half of a bf16 logit's key follows from its sign (0 for a non-negative logit, 0xffff for a negative one, whose
    // ties would otherwise all compare GREATER than T and overflow the sort buffer in arrival order)
    const unsigned T_key = (sizeof(T) == 2 && KEY16 && !shortcut && !(prefix & 0x80000000u)) ? (prefix | 0xffffu) : prefix;
    // ---- ordered compaction into LDS
    if (tid == 0) { s_cnt = 0; s_eqbase = 0; }
    ckey[tid] = 0u;
    cidx[tid] = 0x7fffffff;
    __syncthreads();
    for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
        unsigned kk[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            int n = n0 + j * kSelThreads + tid;
            kk[j] = ld_sel(fk, n, n < N, 0u);
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            int n = n0 + j * kSelThreads + tid;
            unsigned key = kk[j];
            bool gt = n < N && key > T_key, eq = n < N && key == T_key;
            unsigned long long em = __ballot(eq);
            if (__syncthreads_or(eq)) {          // chunks without a tie candidate (almost all) skip the ordered ranking
                if (lane == 0) wsum[wv] = __popcll(em);
                __syncthreads();
                int ebase = s_eqbase;
                for (int w2 = 0; w2 < wv; ++w2) ebase += wsum[w2];
                int erank = ebase + __popcll(em & ((1ull << lane) - 1ull));
                eq = eq && erank < (int)need;
                __syncthreads();
                if (tid == 0) {
                    int tot = 0;
                    for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wsum[w2];
                    s_eqbase += tot;
                }
                __syncthreads();
            }
            if (gt || eq) {
                int pos = atomicAdd(&s_cnt, 1);
                if (pos < kSelThreads) { ckey[pos] = key; cidx[pos] = n; }
            }
        }
    }
    __syncthreads();
    // ---- bitonic sort of the (key desc, idx asc) pairs; unused slots hold key 0 / idx INT_MAX and sink to the end
    for (int size = 2; size <= kSelThreads; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            int partner = tid ^ stride;
            if (partner > tid) {
                unsigned ka = ckey[tid], kb = ckey[partner];
                int ia = cidx[tid], ib = cidx[partner];
                bool a_first = ka > kb || (ka == kb && ia < ib);       // a should precede b in descending order
                bool up = (tid & size) == 0;                            // this run is sorted "descending-first"
                if (up ? !a_first : a_first) {
                    ckey[tid] = kb; ckey[partner] = ka;
                    cidx[tid] = ib; cidx[partner] = ia;
                }
            }
            __syncthreads();
        }
    }
    // ---- outputs
    if (tid < K) {
        int n = cidx[tid];
        float sc = sigmoidf_(key2f(ckey[tid]));
        int lab = 0;
        if (g.nc > 1 && n < N) anchor_key(cls, v, g, b, n, &lab);
        top_idx[(size_t)b * K + tid] = n < N ? n : 0;
        top_score[(size_t)b * K + tid] = sc;
        top_label[(size_t)b * K + tid] = lab;
    }
    // number of selected anchors with score >= threshold (a prefix of the sorted list)
    bool ok = tid < K && cidx[tid] < N && sigmoidf_(key2f(ckey[tid])) >= score_thr;
    unsigned long long m = __ballot(ok);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wsum[w2];
        counts[b] = tot;
    }
}


// ---- register-resident select (frames of up to 1024 * KPT anchors: car.fhd has 70400) ----------------------------------
// k_predict_select walks the frame's key array three times (two radix passes + compaction, 9 dependent load rounds each),
// re-synchronises the workgroup once per 1024 keys to rank ties, and finishes with a 55-barrier bitonic sort.  Here every
// thread loads its KPT keys ONCE (wave-contiguous segments, so "first by index" among equal keys is a prefix over waves),
// the radix passes, tie ranking and compaction run out of registers, and the sort does its in-wave steps with shuffles
// (10 LDS exchange steps instead of 55).  Same outputs as k_predict_select.
// INDIRECT (second stage of the chunked select): `keys` are the per-chunk candidate keys written by k_predict_select_chunk
// (n_keys of them per frame, chunk-major, ascending anchor index among equal keys inside and across chunks -- which is all the
// tie ranking needs), slot_anchor their anchor ids.
template <typename T, int KP, bool INDIRECT = false, typename V = View5>   // 16-bit logits (bf16 / fp16: key16_of); KP = key PAIRS (dwords) per thread
__global__ __launch_bounds__(kSelThreads) void k_predict_select_reg(const T *__restrict__ cls, V v, PredGeom g, int K,
                                                                    float score_thr, const unsigned short *__restrict__ keys,
                                                                    int ns, int *__restrict__ top_idx,
                                                                    float *__restrict__ top_score, int *__restrict__ top_label,
                                                                    int *__restrict__ counts, int n_keys = 0,
                                                                    const int *__restrict__ slot_anchor = nullptr, unsigned thr16 = 0u) {
    __shared__ unsigned ckey[kSelThreads];
    __shared__ int cidx[kSelThreads];
    __shared__ int wsum[kSelThreads / 64];
    __shared__ int wred[2][kSelThreads / 64];
    __shared__ int s_cnt;
    __shared__ unsigned short cand_key[kCandCap];
    __shared__ int cand_idx[kCandCap];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = INDIRECT ? n_keys : g.A * g.H * g.W;
    const unsigned *fk2 = reinterpret_cast<const unsigned *>(keys + (size_t)b * ns);   // ns is even: dword aligned
    if (K > kSelThreads) K = kSelThreads;
    if (K > N) K = N;
    const int n_base = wv * (KP * 128) + lane * 2;    // pair i of this thread = anchors n_base + 128 i and + 1
    unsigned k2[KP];                                  // low half: even anchor's key, high half: the odd one's
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const int n = n_base + i * 128;
        k2[i] = ld_sel(fk2, n >> 1, n < ns, 0u);
    }
    // K-th largest 16-bit key by bisection on its bits, MSB first (no histogram, no atomics).  Counting sweeps run over
    // all registers only while more than CAND_CAP keys lie at or above the current lower bound; then those few are
    // compacted into LDS (two per thread) and the remaining bits are resolved on them.  Out-of-range slots hold key 0
    // and are never counted because every probe is >= 1.
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    auto block_sum = [&](int c, int it) -> int {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) wred[it & 1][wv] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wred[it & 1][w2];
        return tot;
    };
    auto count_ge = [&](unsigned t, int it) -> int {
        // packed 16-bit arithmetic, three VALU ops per key pair: min(1, sat(k - (t - 1))) is 1 exactly when k >= t
        const us2 tm1 = {(unsigned short)(t - 1), (unsigned short)(t - 1)}, one = {1, 1};
        us2 acc2 = {0, 0};
#pragma unroll
        for (int i = 0; i < KP; ++i)
            acc2 += __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_bit_cast(us2, k2[i]), tm1), one);
        return block_sum((int)acc2.x + (int)acc2.y, it);
    };
    unsigned cand = 0;
    int it = 0, bit = 15, above = N;                  // above = number of keys >= cand
    // thr16 (see k_predict_select_chunk): no more than K keys at or above the threshold's key -> they are the selection, no bisection
    bool quick = false;
    if (thr16 > 0u) {
        const int c = count_ge(thr16, it++);
        if (c <= K) { quick = true; cand = thr16; above = c; bit = -1; }
    }
    for (; bit >= 0 && above > kCandCap; --bit, ++it) {
        const unsigned t = cand | (1u << bit);
        const int c = count_ge(t, it);
        if (c >= K) { cand = t; above = c; }
    }
    bool sorted_ready = false;                        // the sort buffer already holds every key >= T (ties included)
    ckey[tid] = 0u;
    cidx[tid] = 0x7fffffff;
    if (quick) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < KP; ++i)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const unsigned kj = (k2[i] >> (hf * 16)) & 0xffffu;
                const int n = n_base + i * 128 + hf;
                const bool hit = n < N && kj >= cand;
                const unsigned long long m = __ballot(hit);
                if (m) {                               // one LDS atomic per wave; the sort orders the slots
                    int p0 = 0;
                    if (lane == 0) p0 = atomicAdd(&s_cnt, __popcll(m));
                    p0 = __shfl(p0, 0, 64);
                    const int pos = p0 + __popcll(m & lt);
                    if (hit && pos < kSelThreads) { ckey[pos] = (kj << 16) | ((kj & 0x8000u) ? 0u : 0xffffu); cidx[pos] = n; }
                }
            }
        sorted_ready = true;
    } else if (bit >= 0) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KP; ++i)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const unsigned kj = (k2[i] >> (hf * 16)) & 0xffffu;
                const int n = n_base + i * 128 + hf;
                if (n < N && kj >= cand) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < kCandCap) { cand_key[pos] = (unsigned short)kj; cand_idx[pos] = n; }
                }
            }
        __syncthreads();
        const int m = s_cnt < kCandCap ? s_cnt : kCandCap;
        unsigned c2[kCandCap / kSelThreads];
        int ci[kCandCap / kSelThreads];
#pragma unroll
        for (int u = 0; u < kCandCap / kSelThreads; ++u) {
            const int p = tid + u * kSelThreads;
            c2[u] = p < m ? (unsigned)cand_key[p] : 0u;
            ci[u] = p < m ? cand_idx[p] : 0x7fffffff;
        }
        auto count_ge_c = [&](unsigned t, int it2) -> int {
            int c = 0;
#pragma unroll
            for (int u = 0; u < kCandCap / kSelThreads; ++u) c += c2[u] >= t ? 1 : 0;
            return block_sum(c, it2);
        };
        for (; bit >= 0; --bit, ++it) {
            const unsigned t = cand | (1u << bit);
            const int c = count_ge_c(t, it);
            if (c >= K) { cand = t; above = c; }
        }
        if (above <= kSelThreads && cand > 0) {       // everything at or above T fits the sort buffer: the sort ranks the ties
            if (tid == 0) s_cnt = 0;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kCandCap / kSelThreads; ++u)
                if (c2[u] >= cand) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    ckey[pos] = (c2[u] << 16) | ((c2[u] & 0x8000u) ? 0u : 0xffffu);
                    cidx[pos] = ci[u];
                }
            sorted_ready = true;
        }
    }
    const unsigned prefix = cand;
    if (!sorted_ready) {
    const unsigned need = cand == 0xffffu ? (unsigned)K : (unsigned)(K - count_ge(cand + 1, it));
    const unsigned T_key = prefix;   // K-th largest (16-bit) key; take all keys > T and the first `need` (by index) equal to T
    // ties: a wave's keys are a contiguous index range (pair i, lane, half = ascending anchor index), so its first tie
    // ranks after all ties of the waves before it
    int my_eq = 0;
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
            my_eq += __popcll(__ballot(n_base + i * 128 + hf < N && ((k2[i] >> (hf * 16)) & 0xffffu) == T_key));
    if (tid == 0) s_cnt = 0;
    if (lane == 0) wsum[wv] = my_eq;
    __syncthreads();
    int erun = 0;
    for (int w2 = 0; w2 < wv; ++w2) erun += wsum[w2];
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const int n = n_base + i * 128;
        const unsigned ka = k2[i] & 0xffffu, kb = k2[i] >> 16;
        const bool eqa = n < N && ka == T_key, eqb = n + 1 < N && kb == T_key;
        const unsigned long long ma = __ballot(eqa), mb = __ballot(eqb);
        const int before = erun + __popcll(ma & lt) + __popcll(mb & lt);
        erun += __popcll(ma) + __popcll(mb);
        const bool ta = (n < N && ka > T_key) || (eqa && before < (int)need);
        const bool tb = (n + 1 < N && kb > T_key) || (eqb && before + (eqa ? 1 : 0) < (int)need);
        // full key: f2key of a 16-bit float has low half 0 (non-negative input) or 0xffff (negative input)
        if (ta) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < kSelThreads) { ckey[pos] = (ka << 16) | ((ka & 0x8000u) ? 0u : 0xffffu); cidx[pos] = n; }
        }
        if (tb) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < kSelThreads) { ckey[pos] = (kb << 16) | ((kb & 0x8000u) ? 0u : 0xffffu); cidx[pos] = n + 1; }
        }
    }
    }   // !sorted_ready
    __syncthreads();
    // ---- bitonic sort of (key desc, idx asc); strides < 64 stay inside the wave (shuffles), the rest go through LDS
    unsigned mk = ckey[tid];
    int mi = cidx[tid];
    for (int size = 2; size <= kSelThreads; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            unsigned ok_;
            int oi;
            if (stride >= 64) {
                __syncthreads();
                ckey[tid] = mk; cidx[tid] = mi;
                __syncthreads();
                ok_ = ckey[tid ^ stride]; oi = cidx[tid ^ stride];
            } else {
                ok_ = (unsigned)__shfl_xor((int)mk, stride, 64);
                oi = __shfl_xor(mi, stride, 64);
            }
            const bool lower = (tid & stride) == 0;                    // this thread holds the first slot of the pair
            const bool mine_first = mk > ok_ || (mk == ok_ && mi < oi);   // my element precedes the partner's (descending)
            const bool up = (tid & size) == 0;                         // this run is sorted descending-first
            const bool keep_mine = (lower == up) ? mine_first : !mine_first;
            if (!keep_mine) { mk = ok_; mi = oi; }
        }
    }
    // ---- outputs
    if (INDIRECT) {                                   // slot -> anchor id (empty candidate slots carry 0x7fffffff)
        const int a_ = (mi < N) ? slot_anchor[(size_t)b * N + mi] : 0x7fffffff;
        mi = (a_ < g.A * g.H * g.W) ? a_ : 0x7fffffff;
    }
    const int n_valid = INDIRECT ? 0x7fffffff : N;    // below: mi < n_valid == a real anchor
    if (tid < K) {
        float sc = mi < n_valid ? sigmoidf_(key16_logit<T>(mk >> 16)) : 0.0f;      // empty slots (fewer than K selected): score 0, anchor 0
        int lab = 0;
        if (g.nc > 1 && mi < n_valid) anchor_key(cls, v, g, b, mi, &lab);
        top_idx[(size_t)b * K + tid] = mi < n_valid ? mi : 0;
        top_score[(size_t)b * K + tid] = sc;
        top_label[(size_t)b * K + tid] = lab;
    }
    const bool ok = tid < K && mi < n_valid && sigmoidf_(key16_logit<T>(mk >> 16)) >= score_thr;
    const unsigned long long m = __ballot(ok);
    __syncthreads();
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wsum[w2];
        counts[b] = tot;
    }
}

// ---- chunked select, stage 1 (whole chip) -------------------------------------------------------------------------------
// One workgroup per (frame, chunk of 8192 anchors): its top-min(K, chunk) keys -- everything above the chunk's K-th largest key
// T plus the first ties at T by anchor index -- written in ASCENDING ANCHOR ORDER (deterministic ballot-prefix slots) to
// cand_key / cand_idx [frame][chunk][1024], zero / 0x7fffffff padded.  The frame's top K is a subset of the union of its chunks'
// top K, with the same tie order, so stage 2 (k_predict_select_reg<INDIRECT>) selects and sorts ~9 k candidates instead of
// bisecting 70 k keys in one workgroup: 65 us -> two launches of ~6 and ~17 us.
constexpr int kSelChunk = 8192;                  // 16 waves x 4 key pairs x 128 (KP = 4)
// Round 3: (a) the keys are computed HERE from the head output (the separate whole-chip k_predict_keys16 launch, 12.5 us, is gone
// from this path; a chunk's 8192 anchors are 8192 scattered 2-byte reads either way); (b) `thr16` > 0 is a 16-bit key at or below
// the key of every logit whose score reaches the caller's threshold (computed conservatively on the host): when no more than K
// keys of the chunk lie at or above it -- the normal case for a trained head: a few hundred candidates per frame -- they ARE the
// chunk's contribution and the 16-step bisection is skipped.  Entries below the threshold can then be missing from the frame's
// top K; they lie behind counts[b] and were never part of the reference's result (voxelnet.py:551-570 masks by the threshold
// before its topk).
// KP = key pairs per thread: 4 (8192-anchor chunks, the usual heads) or 36 (73 728-anchor chunks: heads of > 600 k anchors per
// frame -- nuScenes all.fhd has 1.23 M -- whose 8192-anchor chunks would hand the second stage more candidate slots than it holds).
template <typename T, int KP, typename V = View5>
__global__ __launch_bounds__(kSelThreads) void k_predict_select_chunk(const T *__restrict__ cls, V v, PredGeom g, int N, int K,
                                                                      int chunks, unsigned thr16, unsigned short *__restrict__ cand_key,
                                                                      int *__restrict__ cand_idx) {
    constexpr int kChunk = kSelThreads * 2 * KP;
    __shared__ int sweep_tot[20];
    __shared__ int w_eq[kSelThreads / 64], w_gt[kSelThreads / 64];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int base = c * kChunk;
    const int nloc = min(kChunk, N - base);                            // > 0 by construction of the grid
    const int Kc = K < nloc ? K : nloc;
    const int n_base = wv * (KP * 128) + lane * 2;
    unsigned k2[KP];
    // (a, y, x) of the thread's first anchor by division, of the others by stepping (anchor n = (a * H + y) * W + x): the runtime
    // divisions of anchor_key() were a third of this kernel's instructions
    // segments: the same stepping inside the segment the thread is in (`cur`); a step across a segment border enters the next one by
    // division again (rare), and pointers stand for the offsets because every segment has a base of its own
    constexpr bool SEG = std::is_same<V, SegView>::value;
    int ax = 0, ay = 0, aa = 0;
    SegCur<T> cur{};
    if constexpr (SEG) {
        const int n0 = base + n_base;
        seg_enter(v, b, n0 < N ? n0 : 0, cur, ax, ay, aa);
    } else {
        const int n0 = base + n_base;
        ax = n0 % g.W;
        const int t0 = n0 / g.W;
        ay = t0 % g.H;
        aa = t0 / g.H;
    }
    // Offsets first, then the loads of a batch of four pairs back to back (an anchor past the frame reads element 0 and its key is
    // forced to 0 afterwards): `a0 < N ? load : 0` compiles to a branch with s_waitcnt vmcnt(0) behind every load -- eight dependent
    // round trips per thread at KP = 4, most of this kernel's 18 us.
    constexpr int PB = KP < 4 ? KP : 4;
    static_assert(KP % PB == 0, "pairs per thread must be a multiple of the load batch");
#pragma unroll
    for (int i0 = 0; i0 < KP; i0 += PB) {
        long long off[2 * PB];
        bool ok[2 * PB], keep[2 * PB];
        const T *src[2 * PB];
        long long csc[2 * PB];
        if constexpr (SEG) {
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const int a0 = base + n_base + (i0 + j) * 128;          // a0 < N: `cur` is a0's segment and (aa, ay, ax) its place there
                ok[2 * j] = a0 < N;
                ok[2 * j + 1] = a0 + 1 < N;
                src[2 * j] = ok[2 * j] ? cur.frame + aa * cur.sa + ay * cur.sy + ax * cur.sx : cur.frame;
                csc[2 * j] = csc[2 * j + 1] = cur.sc;
                if (ok[2 * j + 1] && a0 + 1 >= cur.end) {                // the pair straddles a segment border
                    src[2 * j + 1] = seg_anchor<T>(v, b, a0 + 1, &csc[2 * j + 1]);
                } else {
                    int bx = ax + 1, by = ay, ba = aa;
                    if (bx >= cur.W) { bx = 0; if (++by >= cur.H) { by = 0; ++ba; } }
                    src[2 * j + 1] = ok[2 * j + 1] ? cur.frame + ba * cur.sa + by * cur.sy + bx * cur.sx : cur.frame;
                }
                const int an = a0 + 128;                                 // the thread's next pair
                if (an < N && an >= cur.end) {
                    seg_enter(v, b, an, cur, ax, ay, aa);
                } else {
                    ax += 128;
                    while (ax >= cur.W) { ax -= cur.W; if (++ay >= cur.H) { ay = 0; ++aa; } }
                }
            }
        } else {
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int a0 = base + n_base + (i0 + j) * 128;
            int bx = ax + 1, by = ay, ba = aa;             // the pair's second anchor
            if (bx >= g.W) { bx = 0; if (++by >= g.H) { by = 0; ++ba; } }
            ok[2 * j] = a0 < N;
            ok[2 * j + 1] = a0 + 1 < N;                                 // slots beyond the frame hold key 0
            off[2 * j] = ok[2 * j] ? frame_off(v, b, ay, ax) + (long long)aa * v.sa + (long long)ay * v.sy + (long long)ax * v.sx : 0;
            off[2 * j + 1] = ok[2 * j + 1] ? frame_off(v, b, by, bx) + (long long)ba * v.sa + (long long)by * v.sy + (long long)bx * v.sx : 0;
            ax += 128;
            while (ax >= g.W) { ax -= g.W; if (++ay >= g.H) { ay = 0; ++aa; } }
        }
        }
#pragma unroll
        for (int j = 0; j < 2 * PB; ++j) keep[j] = ok[j];
        if constexpr (!SEG) if (v.amask) {                               // as anchor_key(): a masked-out anchor holds key 0 too
            unsigned char m[2 * PB];
#pragma unroll
            for (int j = 0; j < 2 * PB; ++j)
                m[j] = v.amask[ok[j] ? (long long)b * N + base + n_base + (i0 + j / 2) * 128 + (j & 1) : 0];
#pragma unroll
            for (int j = 0; j < 2 * PB; ++j) keep[j] = ok[j] && m[j] != 0;
        }
        float best[2 * PB];
#pragma unroll
        for (int j = 0; j < 2 * PB; ++j) {
            if constexpr (SEG) best[j] = ldf(src[j]);
            else best[j] = ldf(cls + off[j]);
        }
        for (int c2 = 1; c2 < g.nc; ++c2) {                              // as anchor_key()
            float f[2 * PB];
#pragma unroll
            for (int j = 0; j < 2 * PB; ++j) {
                if constexpr (SEG) f[j] = ldf(src[j] + (ok[j] ? (long long)c2 * csc[j] : 0));
                else f[j] = ldf(cls + off[j] + (ok[j] ? (long long)c2 * v.sc : 0));
            }
#pragma unroll
            for (int j = 0; j < 2 * PB; ++j) if (f[j] > best[j] || f[j] != f[j]) best[j] = f[j];
        }
#pragma unroll
        for (int j = 0; j < 2 * PB; ++j) keep[j] = keep[j] && best[j] == best[j];   // as anchor_key(): a NaN maximum holds key 0
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const unsigned ka = keep[2 * j] ? key16_of<T>(best[2 * j]) : 0u;
            const unsigned kb = keep[2 * j + 1] ? key16_of<T>(best[2 * j + 1]) : 0u;
            k2[i0 + j] = ka | (kb << 16);
        }
    }
    unsigned short *ok_ = cand_key + ((size_t)b * chunks + c) * kSelThreads;
    int *oi_ = cand_idx + ((size_t)b * chunks + c) * kSelThreads;
    ok_[tid] = 0;
    oi_[tid] = 0x7fffffff;
    if (tid < 20) sweep_tot[tid] = 0;
    __syncthreads();
    auto block_sum = [&](int x, int it) -> int {
        x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
        x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
        x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, true);    // row_half_mirror
        x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, true);    // row_mirror
        const int ws_ = __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
                        __builtin_amdgcn_readlane(x, 48);
        if (lane == 0) atomicAdd(&sweep_tot[it], ws_);
        __syncthreads();
        return sweep_tot[it];
    };
    auto count_ge = [&](unsigned t, int it) -> int {
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < KP; ++i) cnt += ((k2[i] & 0xffffu) >= t ? 1 : 0) + ((k2[i] >> 16) >= t ? 1 : 0);
        return block_sum(cnt, it);
    };
    unsigned T_key = 0;
    int it = 0;
    bool quick = false;
    if (thr16 > 0u) {
        quick = count_ge(thr16, it++) <= Kc;
        if (quick) T_key = thr16;
    }
    if (!quick)
        for (int bit = 15; bit >= 0; --bit, ++it) {
            const unsigned t = T_key | (1u << bit);
            if (count_ge(t, it) >= Kc) T_key = t;
        }
    const int above = T_key == 0xffffu ? 0 : count_ge(T_key + 1, it);
    const int need = Kc - above;                                          // ties at T to keep, by ascending anchor index
    int my_eq = 0, my_gt = 0;
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const unsigned kj = (k2[i] >> (hf * 16)) & 0xffffu;
            my_eq += __popcll(__ballot(kj == T_key));
            my_gt += __popcll(__ballot(kj > T_key));
        }
    if (lane == 0) { w_eq[wv] = my_eq; w_gt[wv] = my_gt; }
    __syncthreads();
    int erun = 0, slot = 0;
    for (int w2 = 0; w2 < wv; ++w2) {
        const int left = need - erun;
        slot += w_gt[w2] + (left <= 0 ? 0 : (left < w_eq[w2] ? left : w_eq[w2]));
        erun += w_eq[w2];
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const int n = n_base + i * 128;
        const unsigned ka = k2[i] & 0xffffu, kb = k2[i] >> 16;
        const bool eqa = ka == T_key, eqb = kb == T_key;
        const unsigned long long ma = __ballot(eqa), mb = __ballot(eqb);
        const int before = erun + __popcll(ma & lt) + __popcll(mb & lt);
        erun += __popcll(ma) + __popcll(mb);
        const bool ta = ka > T_key || (eqa && before < need);
        const bool tb = kb > T_key || (eqb && before + (eqa ? 1 : 0) < need);
        const unsigned long long qa = __ballot(ta), qb = __ballot(tb);
        const unsigned long long both_lt = lt;
        // ascending anchor order inside the pair row: lane L's two anchors (2L, 2L + 1) come before lane L + 1's
        const int pa = slot + __popcll(qa & both_lt) + __popcll(qb & both_lt);
        const int pb = pa + (ta ? 1 : 0);
        slot += __popcll(qa) + __popcll(qb);
        if (ta && pa < kSelThreads) { ok_[pa] = (unsigned short)ka; oi_[pa] = base + n; }
        if (tb && pb < kSelThreads) { ok_[pb] = (unsigned short)kb; oi_[pb] = base + n + 1; }
    }
}

// The decode of one selected box.  WIDE = false: rows of 7 values (k_predict_decode).  WIDE = true: rows of nd = 7 + custom_ndim
// values (k_predict_decode_nd; GroundBox3dCoder with custom_ndim > 0, box_torch_ops.py:15-102): columns 0-6 by the same expressions,
// column 7 + j = encoding + anchor; dets and dir_label never see the custom columns.
template <typename T, typename V, bool WIDE>
__device__ __forceinline__ void predict_decode_row(const T *__restrict__ box, const V &vb, const T *__restrict__ dir,
                                                   const V &vd, int ndir, const PredGeom &g, int K,
                                                   const float *__restrict__ anchors, const int *__restrict__ top_idx,
                                                   const float *__restrict__ top_score, int rotate,
                                                   float *__restrict__ dec, float *__restrict__ dets,
                                                   int *__restrict__ dir_label, int nd_arg) {
    const int nd = WIDE ? nd_arg : 7;          // row pitch of anchors and dec
    int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.batch * K) return;
    int b = t / K;
    int n = top_idx[t];
    constexpr bool SEG = std::is_same<V, SegView>::value;
    int x = 0, y = 0, a = 0;
    const T *pb;
    long long bsc;
    if constexpr (SEG) {
        pb = seg_anchor<T>(vb, b, n, &bsc);
    } else {
        x = n % g.W;
        int q = n / g.W;
        y = q % g.H;
        a = q / g.H;
        pb = box + frame_off(vb, b, y, x) + a * vb.sa + y * vb.sy + x * vb.sx;
        bsc = vb.sc;
    }
    float e[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) e[c] = ldf(pb + c * bsc);
    const float *an = anchors + (size_t)n * nd;
    float xa = an[0], ya = an[1], za = an[2], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    float diag = sqrtf(__fadd_rn(__fmul_rn(la, la), __fmul_rn(wa, wa)));
    float o[7];
    o[0] = __fadd_rn(__fmul_rn(e[0], diag), xa);
    o[1] = __fadd_rn(__fmul_rn(e[1], diag), ya);
    o[2] = __fadd_rn(__fmul_rn(e[2], ha), za);
    o[3] = __fmul_rn(expf(e[3]), wa);
    o[4] = __fmul_rn(expf(e[4]), la);
    o[5] = __fmul_rn(expf(e[5]), ha);
    o[6] = __fadd_rn(e[6], ra);
#pragma unroll
    for (int c = 0; c < 7; ++c) dec[(size_t)t * nd + c] = o[c];
    if constexpr (WIDE)
        for (int c = 7; c < nd; ++c) dec[(size_t)t * nd + c] = __fadd_rn(ldf(pb + c * bsc), an[c]);
    float *d = dets + (size_t)t * 6;
    if (rotate) {        // boxes_for_nms = box[:, [0, 1, 3, 4, 6]] + score
        d[0] = o[0]; d[1] = o[1]; d[2] = o[3]; d[3] = o[4]; d[4] = o[6]; d[5] = top_score[t];
    } else {             // standup box of the rotated BEV rectangle (center_to_corner_box2d + corner_to_standup_nd)
        float hx = o[3] * 0.5f, hy = o[4] * 0.5f;
        float cs = fabsf(cosf(o[6])), sn = fabsf(sinf(o[6]));
        float ex = hx * cs + hy * sn, ey = hx * sn + hy * cs;
        d[0] = o[0] - ex; d[1] = o[1] - ey; d[2] = o[0] + ex; d[3] = o[1] + ey; d[4] = top_score[t]; d[5] = 0.0f;
    }
    int dl = 0;
    if (dir) {
        const T *pd;
        long long dsc;
        if constexpr (SEG) {
            pd = seg_anchor<T>(vd, b, n, &dsc);
        } else {
            pd = dir + frame_off(vd, b, y, x) + a * vd.sa + y * vd.sy + x * vd.sx;
            dsc = vd.sc;
        }
        float best = ldf(pd);
        for (int c = 1; c < ndir; ++c) {
            float f = ldf(pd + c * dsc);
            if (f > best) { best = f; dl = c; }
        }
    }
    dir_label[t] = dl;
}

template <typename T, typename V = View5>
__global__ __launch_bounds__(kBlock) void k_predict_decode(const T *__restrict__ box, V vb, const T *__restrict__ dir,
                                                          V vd, int ndir, PredGeom g, int K,
                                                          const float *__restrict__ anchors, const int *__restrict__ top_idx,
                                                          const float *__restrict__ top_score, int rotate,
                                                          float *__restrict__ dec, float *__restrict__ dets,
                                                          int *__restrict__ dir_label) {
    predict_decode_row<T, V, false>(box, vb, dir, vd, ndir, g, K, anchors, top_idx, top_score, rotate, dec, dets, dir_label, 7);
}
template <typename T, typename V = View5>
__global__ __launch_bounds__(kBlock) void k_predict_decode_nd(const T *__restrict__ box, V vb, const T *__restrict__ dir,
                                                             V vd, int ndir, PredGeom g, int K,
                                                             const float *__restrict__ anchors, const int *__restrict__ top_idx,
                                                             const float *__restrict__ top_score, int rotate,
                                                             float *__restrict__ dec, float *__restrict__ dets,
                                                             int *__restrict__ dir_label, int nd) {
    predict_decode_row<T, V, true>(box, vb, dir, vd, ndir, g, K, anchors, top_idx, top_score, rotate, dec, dets, dir_label, nd);
}

// WIDE as in predict_decode_row: the direction fix on column 6, the range mask on columns 0-2, custom columns copied
template <bool WIDE>
__device__ __forceinline__ void predict_finalize_row(const float *__restrict__ dec, const float *__restrict__ top_score,
                                                     const int *__restrict__ top_label, const int *__restrict__ dir_label,
                                                     const int *__restrict__ keep, const int *__restrict__ num_keep,
                                                     int batch, int K, int P, int use_dir, float dir_offset,
                                                     float dir_limit_offset, float period, const float *__restrict__ range6,
                                                     float *__restrict__ boxes, float *__restrict__ scores,
                                                     int *__restrict__ labels, unsigned char *__restrict__ valid, int nd_arg) {
    const int nd = WIDE ? nd_arg : 7;
    int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= batch * P) return;
    int b = t / P, j = t - b * P;
    bool ok = j < num_keep[b];
    int sel = ok ? keep[(size_t)b * K + j] : 0;
    const float *s = dec + ((size_t)b * K + sel) * nd;
    float o[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = s[c];
    if (use_dir) {   // limit_period(rot - offset, limit_offset, period) + offset + period * dir_label
        float val = __fsub_rn(o[6], dir_offset);
        float rot = __fsub_rn(val, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(val, period), dir_limit_offset)), period));
        o[6] = __fadd_rn(__fadd_rn(rot, dir_offset), __fmul_rn(period, (float)dir_label[(size_t)b * K + sel]));
    }
    if (range6)
        ok = ok && o[0] >= range6[0] && o[1] >= range6[1] && o[2] >= range6[2] && o[0] <= range6[3] && o[1] <= range6[4] &&
             o[2] <= range6[5];
#pragma unroll
    for (int c = 0; c < 7; ++c) boxes[(size_t)t * nd + c] = o[c];
    if constexpr (WIDE)
        for (int c = 7; c < nd; ++c) boxes[(size_t)t * nd + c] = s[c];
    scores[t] = top_score[(size_t)b * K + sel];
    labels[t] = top_label[(size_t)b * K + sel];
    valid[t] = ok ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void k_predict_finalize(const float *__restrict__ dec, const float *__restrict__ top_score,
                                                            const int *__restrict__ top_label, const int *__restrict__ dir_label,
                                                            const int *__restrict__ keep, const int *__restrict__ num_keep,
                                                            int batch, int K, int P, int use_dir, float dir_offset,
                                                            float dir_limit_offset, float period, const float *__restrict__ range6,
                                                            float *__restrict__ boxes, float *__restrict__ scores,
                                                            int *__restrict__ labels, unsigned char *__restrict__ valid) {
    predict_finalize_row<false>(dec, top_score, top_label, dir_label, keep, num_keep, batch, K, P, use_dir, dir_offset, dir_limit_offset, period,
                                range6, boxes, scores, labels, valid, 7);
}
__global__ __launch_bounds__(kBlock) void k_predict_finalize_nd(const float *__restrict__ dec, const float *__restrict__ top_score,
                                                               const int *__restrict__ top_label, const int *__restrict__ dir_label,
                                                               const int *__restrict__ keep, const int *__restrict__ num_keep,
                                                               int batch, int K, int P, int use_dir, float dir_offset,
                                                               float dir_limit_offset, float period, const float *__restrict__ range6,
                                                               float *__restrict__ boxes, float *__restrict__ scores,
                                                               int *__restrict__ labels, unsigned char *__restrict__ valid, int nd) {
    predict_finalize_row<true>(dec, top_score, top_label, dir_label, keep, num_keep, batch, K, P, use_dir, dir_offset, dir_limit_offset, period,
                               range6, boxes, scores, labels, valid, nd);
}

// ---- multi-class NMS (voxelnet.py:458-547): (frame, class) items ------------------------------------------------------------
// Class c of a frame selects among the anchors of ITS a-range [a_begin, a_end) (all anchors when class-agnostic) by the sigmoid of
// column c alone, with its own threshold and k.  One workgroup per item; gridDim.x = classes, so the workgroups that read a frame's
// cls rows through different columns are dispatched together and share the rows' cache lines in L2 (a channels-last head keeps the
// A * C logits of a pixel in one or two lines).
// The result of an item is what k_predict_select / k_predict_select_reg return for the one-class strided view of the same tensor:
// entries ordered by (key descending, anchor index ascending), the first min(k, anchors) of them, counts = those whose score reaches
// the threshold.  Because the threshold is > 0 here (checked on the host), only passing anchors are ever candidates:
//   common case: at most 1024 anchors pass -- ONE sweep over the head compacts them into LDS, the sort ranks them;
//   otherwise: the radix select of k_predict_select over the passing anchors (four histogram sweeps, ordered tie ranking), re-reading
//   the head (L2 resident) instead of a key array.
constexpr int kMaxSelClasses = 32;
struct ClassSel {                      // per-class host settings, by value in the kernel argument (read with a uniform index)
    int a_begin[kMaxSelClasses], a_end[kMaxSelClasses], k[kMaxSelClasses];
    float thr[kMaxSelClasses];
};

template <typename T>
__global__ __launch_bounds__(kSelThreads) void k_predict_select_classes(const T *__restrict__ cls, View5 v, PredGeom g, ClassSel p, int Kout,
                                                                        int *__restrict__ top_idx, float *__restrict__ top_score,
                                                                        int *__restrict__ counts) {
    __shared__ unsigned hist[256];
    __shared__ unsigned ckey[kSelThreads];
    __shared__ int cidx[kSelThreads];
    __shared__ int wsum[kSelThreads / 64];
    __shared__ unsigned s_prefix, s_need;
    __shared__ int s_cnt, s_eqbase;
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int HW = g.H * g.W;
    const int first = p.a_begin[c] * HW;                 // the item's anchors: [first, first + N) of the frame's list
    const int N = (p.a_end[c] - p.a_begin[c]) * HW;
    const float thr = p.thr[c];
    int K = p.k[c];
    if (K > kSelThreads) K = kSelThreads;
    if (K > N) K = N;
    const T *frame = cls + (long long)b * v.sb + (long long)c * v.sc;
    constexpr int UNR = 4;                               // independent logit loads in flight per thread
    // key of local anchor n (0: past the range, or below the threshold -- never a candidate)
    auto load_keys = [&](int n0, unsigned (&kk)[UNR]) {
        float f[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int n = n0 + j * kSelThreads + tid;
            const int m = (n < N ? n : 0) + first;
            const int x = m % g.W, t = m / g.W, y = t % g.H, a = t / g.H;
            f[j] = ldf(frame + (long long)a * v.sa + (long long)y * v.sy + (long long)x * v.sx);
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int n = n0 + j * kSelThreads + tid;
            kk[j] = (n < N && sigmoidf_(f[j]) >= thr) ? f2key(f[j]) : 0u;
        }
    };
    if (tid == 0) { s_cnt = 0; s_eqbase = 0; }
    ckey[tid] = 0u;
    cidx[tid] = 0x7fffffff;
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    // ---- sweep 1: every passing anchor into the sort buffer (slots in arrival order: the sort ranks them), and their number
    for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
        unsigned kk[UNR];
        load_keys(n0, kk);
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const bool hit = kk[j] != 0u;
            const unsigned long long m = __ballot(hit);
            if (m) {                                      // one LDS atomic per wave
                int p0 = 0;
                if (lane == 0) p0 = atomicAdd(&s_cnt, __popcll(m));
                p0 = __shfl(p0, 0, 64);
                const int pos = p0 + __popcll(m & lt);
                if (hit && pos < kSelThreads) { ckey[pos] = kk[j]; cidx[pos] = n0 + j * kSelThreads + tid; }
            }
        }
    }
    __syncthreads();
    const int passing = s_cnt;
    __syncthreads();
    if (passing > kSelThreads) {
        // ---- more candidates than the sort buffer holds: K-th largest key by radix select (8 bits per sweep, MSB first)
        unsigned prefix = 0, mask = 0, need = K;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += kSelThreads) hist[i] = 0;
            __syncthreads();
            for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
                unsigned kk[UNR];
                load_keys(n0, kk);
#pragma unroll
                for (int j = 0; j < UNR; ++j) {
                    const bool act = kk[j] != 0u && (kk[j] & mask) == prefix;
                    const unsigned d = (kk[j] >> shift) & 255u;
                    unsigned long long todo = __ballot(act);     // wave-aggregated: the leading bytes take a handful of values
                    while (todo) {
                        const int leader = __ffsll((long long)todo) - 1;
                        const unsigned d0 = __shfl(d, leader, 64);
                        const unsigned long long same = __ballot(act && d == d0) & todo;
                        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
                        todo &= ~same;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) {
                unsigned acc = 0;
                int bin = 255;
                for (; bin > 0; --bin) {
                    if (acc + hist[bin] >= need) break;
                    acc += hist[bin];
                }
                s_prefix = prefix | ((unsigned)bin << shift);
                s_need = need - acc;                      // how many still to take inside this bin
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
            mask |= 255u << shift;
            __syncthreads();
        }
        const unsigned T_key = prefix;                    // take all keys > T and the first `need` (by index) equal to T
        if (tid == 0) { s_cnt = 0; s_eqbase = 0; }
        ckey[tid] = 0u;
        cidx[tid] = 0x7fffffff;
        __syncthreads();
        for (int n0 = 0; n0 < N; n0 += kSelThreads * UNR) {
            unsigned kk[UNR];
            load_keys(n0, kk);
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                const unsigned key = kk[j];
                const bool gt = key > T_key;              // (T_key > 0: the K-th of more than K passing keys)
                bool eq = key == T_key;
                const unsigned long long em = __ballot(eq);
                if (__syncthreads_or(eq)) {               // chunks without a tie candidate (almost all) skip the ordered ranking
                    if (lane == 0) wsum[wv] = __popcll(em);
                    __syncthreads();
                    int ebase = s_eqbase;
                    for (int w2 = 0; w2 < wv; ++w2) ebase += wsum[w2];
                    const int erank = ebase + __popcll(em & lt);
                    eq = eq && erank < (int)need;
                    __syncthreads();
                    if (tid == 0) {
                        int tot = 0;
                        for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wsum[w2];
                        s_eqbase += tot;
                    }
                    __syncthreads();
                }
                if (gt || eq) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < kSelThreads) { ckey[pos] = key; cidx[pos] = n0 + j * kSelThreads + tid; }
                }
            }
        }
        __syncthreads();
    }
    // ---- bitonic sort of (key desc, idx asc); strides < 64 stay inside the wave (shuffles), the rest go through LDS.  Unused slots
    //      hold key 0 / idx INT_MAX and sink to the end.
    unsigned mk = ckey[tid];
    int mi = cidx[tid];
    for (int size = 2; size <= kSelThreads; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            unsigned ok_;
            int oi;
            if (stride >= 64) {
                __syncthreads();
                ckey[tid] = mk; cidx[tid] = mi;
                __syncthreads();
                ok_ = ckey[tid ^ stride]; oi = cidx[tid ^ stride];
            } else {
                ok_ = (unsigned)__shfl_xor((int)mk, stride, 64);
                oi = __shfl_xor(mi, stride, 64);
            }
            const bool lower = (tid & stride) == 0;
            const bool mine_first = mk > ok_ || (mk == ok_ && mi < oi);
            const bool up = (tid & size) == 0;
            const bool keep_mine = (lower == up) ? mine_first : !mine_first;
            if (!keep_mine) { mk = ok_; mi = oi; }
        }
    }
    // ---- outputs: rows [0, counts) are the selection; the rows behind them hold anchor 0 / score 0
    const bool live = tid < K && mk != 0u;
    if (tid < Kout) {
        const size_t o = ((size_t)b * gridDim.x + c) * Kout + tid;
        top_idx[o] = live ? first + mi : 0;
        top_score[o] = live ? sigmoidf_(key2f(mk)) : 0.0f;
    }
    const unsigned long long m = __ballot(live);
    __syncthreads();
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w2 = 0; w2 < kSelThreads / 64; ++w2) tot += wsum[w2];
        counts[b * gridDim.x + c] = tot;
    }
}

// survivors of the per-item NMS, class after class: output row j of a frame belongs to the class c with post_off[c] <= j < post_off[c + 1]
// and is that class's (j - post_off[c])-th kept candidate; label = c.  Direction fix and range mask as k_predict_finalize.
__global__ __launch_bounds__(kBlock) void k_predict_finalize_classes(const float *__restrict__ dec, const float *__restrict__ top_score,
                                                                    const int *__restrict__ dir_label, const int *__restrict__ keep,
                                                                    const int *__restrict__ num_keep, const int *__restrict__ post_off,
                                                                    int batch, int C, int K, int P, int use_dir, float dir_offset,
                                                                    float dir_limit_offset, float period, const float *__restrict__ range6,
                                                                    float *__restrict__ boxes, float *__restrict__ scores,
                                                                    int *__restrict__ labels, unsigned char *__restrict__ valid) {
    int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= batch * P) return;
    int b = t / P, j = t - b * P;
    int c = 0;
    while (c + 1 < C && j >= post_off[c + 1]) ++c;
    const int r = j - post_off[c];
    const size_t item = (size_t)b * C + c;
    bool ok = r < num_keep[item];
    int sel = ok ? keep[item * K + r] : 0;
    const size_t row = item * K + sel;
    const float *s = dec + row * 7;
    float o[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) o[q] = s[q];
    if (use_dir) {   // limit_period(rot - offset, limit_offset, period) + offset + period * dir_label
        float val = __fsub_rn(o[6], dir_offset);
        float rot = __fsub_rn(val, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(val, period), dir_limit_offset)), period));
        o[6] = __fadd_rn(__fadd_rn(rot, dir_offset), __fmul_rn(period, (float)dir_label[row]));
    }
    if (range6)
        ok = ok && o[0] >= range6[0] && o[1] >= range6[1] && o[2] >= range6[2] && o[0] <= range6[3] && o[1] <= range6[4] &&
             o[2] <= range6[5];
#pragma unroll
    for (int q = 0; q < 7; ++q) boxes[(size_t)t * 7 + q] = o[q];
    scores[t] = top_score[row];
    labels[t] = c;
    valid[t] = ok ? 1 : 0;
}

}  // namespace sec

using namespace sec;

// ---- host side: head forms, the select decision, one launcher per stage, thin entry points ----------------------------------
static View5 mkview(const int64_t *s) { return View5{s[0], s[1], s[2], s[3], s[4], 0, nullptr, 0, 0, nullptr, nullptr, 0, 0}; }
static int elt_bytes(int dtype) { return dtype == SEC_F32 ? 4 : 2; }
static bool dtype_ok(int dtype) { return dtype >= SEC_F32 && dtype <= SEC_BF16; }

// How the producer left a head tensor, and which anchors take part.  All NULL: an EAGER head.  tile_live: TILE-LAZY (bit 4 of
// tile_live[b][tile] = the 8 x 16 tile was written).  cover_cols: COVER-LAZY (a bit per pixel column and 8-row band).  A lazy head
// reads every unwritten element from the empty frame's map: `background` for the cls (select) / box (decode) view, `dir_background`
// for the decode's direction view.  anchor_mask: the MASKED select (on any of the three).
struct HeadForm {
    const unsigned short *tile_live; const unsigned *cover_cols; const void *background, *dir_background; const unsigned char *anchor_mask;
};
// the View5 of one view of such a head (`base` its pointer, `background` the same element of the empty frame's map); SEC_E_INVALID
// for both lazy forms at once, a lazy form without its background or a background without a lazy form
static int head_view(const HeadForm &f, const int64_t *strides5, const void *base, const void *background, int h, int w, int dtype, View5 *out) {
    if ((f.tile_live && f.cover_cols) || (f.tile_live != nullptr || f.cover_cols != nullptr) != (background != nullptr)) return SEC_E_INVALID;
    View5 v = mkview(strides5);
    if (background) v.bg = (long long)((const char *)background - (const char *)base) / elt_bytes(dtype);
    if (f.cover_cols) { v.cover = f.cover_cols; v.cwr = (w + 31) / 32; v.cbands = (h + 7) / 8; }
    else if (f.tile_live) { v.live = f.tile_live; v.tiles_x = (w + 15) / 16; v.tpf = ((h + 7) / 8) * v.tiles_x; }
    v.amask = f.anchor_mask;
    *out = v;
    return SEC_OK;
}

static unsigned ordered_key(float x) {               // f2key() on the host
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// 32-bit key of a logit safely below the score threshold's (k_predict_select's shortcut; 0: none)
static unsigned conservative_thr32(float thr) {
    if (!(thr > 0.0f) || !(thr < 1.0f)) return 0u;
    const float x = logf(thr / (1.0f - thr));
    return ordered_key(x - (fabsf(x) * 1e-4f + 1e-5f));
}
// a 16-bit key no larger than the key of any bf16 logit whose sigmoid reaches `thr` (0 = no such bound): the logit of thr, lowered
// by more than bf16's and sigmoidf's rounding, mapped like f2key() >> 16, minus one key step (truncation of a negative value's
// bits rounds it UP)
static unsigned conservative_thr16(float thr, int dtype) {
    if (!(thr > 0.0f) || !(thr < 1.0f)) return 0u;
    float x = logf(thr / (1.0f - thr));
    x -= fabsf(x) / 64.0f + 0.01f;
    unsigned k16 = ordered_key(x) >> 16;
    if (dtype == SEC_F16) {                          // key16_of<__half>: the sign trick on the half's own bits
        if (!(fabsf(x) < 60000.0f)) return 0u;
        const unsigned u = __half_as_ushort(__float2half_rn(x));
        k16 = (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
    }
    return k16 > 2u ? k16 - 2u : 0u;                 // two key steps down: covers the rounding of the conversions above
}

// ---- the select decision, by anchors per frame and dtype; the names are those of sec_predict_select_plan_name ---------------------
//   radix32        fp32 heads: k_predict_keys + k_predict_select<float, false>, an 8-bit radix select on 32-bit keys
//   direct         16-bit heads of up to kSelChunk = 8192 anchors: k_predict_keys16 + one k_predict_select_reg<T, 36> workgroup per frame
//   chunkKP+kpKP2  larger ones: per-chunk top-K on the whole chip (k_predict_select_chunk<T, KP>: chunks of 8192 anchors, KP 4, while their
//                  candidate lists fit the second stage; of 73 728 anchors, KP 36, up to 5.3 M anchors per frame), then one workgroup per
//                  frame over the chunks * 1024 candidates (k_predict_select_reg<T, KP2, INDIRECT>, KP2 = 5 / 10 / 20 / 36 key pairs per thread)
//   radix16        16-bit heads above that: the radix select OF A 16-BIT HEAD.  Its kernels are the 32-bit-key ones of radix32:
//                  k_predict_select<bf16, true> (two passes, over the high half of the key) and k_predict_select<__half, false>
enum class SelectForm { kRefused, kRadix32, kRadix16, kDirect, kChunked };
struct SelectPlan { SelectForm form; int kp, chunks, kp2; };   // of kChunked only: first-stage KP (4 / 36), its chunk count, second-stage KP2
constexpr long long kSelRegCap = (long long)kSelThreads * 72;   // keys one workgroup of k_predict_select_reg holds (KP 36)

static SelectPlan predict_select_decide(long long n /* anchors per frame */, int dtype) {
    if (dtype == SEC_F32) return {SelectForm::kRadix32, 0, 0, 0};
    if (dtype != SEC_BF16 && dtype != SEC_F16) return {SelectForm::kRefused, 0, 0, 0};
    const long long c4 = (n + kSelChunk - 1) / kSelChunk, c36 = (n + kSelRegCap - 1) / kSelRegCap;
    SelectPlan p{SelectForm::kChunked, 0, 0, 0};
    if (c4 >= 2 && c4 * kSelThreads <= kSelRegCap) { p.kp = 4; p.chunks = (int)c4; }
    else if (n > kSelRegCap && c36 * kSelThreads <= kSelRegCap) { p.kp = 36; p.chunks = (int)c36; }
    else return {n <= kSelRegCap ? SelectForm::kDirect : SelectForm::kRadix16, 0, 0, 0};
    const int pairs = (p.chunks + 1) / 2;            // key pairs per second-stage thread: chunks * 1024 candidates / 2 / 1024 threads
    p.kp2 = pairs <= 5 ? 5 : pairs <= 10 ? 10 : pairs <= 20 ? 20 : 36;
    return p;
}

SEC_API const char *sec_predict_select_plan_name(long long anchors_per_frame, int dtype, int *chunks) {
    static const char *const plain[] = {"", "radix32", "radix16", "direct"};          // indexed by SelectForm
    static const char *const chunked[2][4] = {{"chunk4+kp5", "chunk4+kp10", "chunk4+kp20", "chunk4+kp36"},
                                              {"chunk36+kp5", "chunk36+kp10", "chunk36+kp20", "chunk36+kp36"}};
    const SelectPlan p = predict_select_decide(anchors_per_frame, dtype);
    if (chunks) *chunks = p.chunks;
    return p.form == SelectForm::kChunked ? chunked[p.kp == 36][p.kp2 == 5 ? 0 : p.kp2 == 10 ? 1 : p.kp2 == 20 ? 2 : 3] : plain[(int)p.form];
}

struct SelectArgs {                                  // what every select entry point takes besides its head(s)
    int k; float score_thr; unsigned *key_scratch; int *top_idx; float *top_score; int *top_label, *counts; int dtype; hipStream_t st;
};
template <int N> using Int = std::integral_constant<int, N>;

// the select of a validated call; V = View5 (one head tensor, g = its geometry) or SegView (cls unused, g.A * g.H * g.W = all anchors)
template <typename V>
static int predict_select_launch(const void *cls, const V &v, const PredGeom &g, const SelectArgs &a) {
    const long long nfr = (long long)g.A * g.H * g.W;
    const SelectPlan plan = predict_select_decide(nfr, a.dtype);
    if (plan.form == SelectForm::kRefused) return SEC_E_UNSUPPORTED;
    const dim3 frames(g.batch), wg(kSelThreads);
    return by_dtype(a.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const T *c = (const T *)cls;
        if (plan.form == SelectForm::kRadix32 || plan.form == SelectForm::kRadix16) {
            constexpr bool kKey16 = std::is_same<T, __hip_bfloat16>::value;
            hipLaunchKernelGGL((k_predict_keys<T, V>), dim3(div_up((long long)g.batch * nfr, kBlock)), dim3(kBlock), 0, a.st, c, v, g, a.key_scratch);
            hipLaunchKernelGGL((k_predict_select<T, kKey16, V>), frames, wg, 0, a.st, c, v, g, a.k, a.score_thr, a.key_scratch, a.top_idx,
                               a.top_score, a.top_label, a.counts, conservative_thr32(a.score_thr));
        } else if constexpr (!std::is_same<T, float>::value) {      // (the 16-bit forms have no fp32 instantiation)
            const unsigned thr16 = conservative_thr16(a.score_thr, a.dtype);
            if (plan.form == SelectForm::kDirect) {
                const int ns = (int)((nfr + 1) & ~1ll);
                unsigned short *keys16 = reinterpret_cast<unsigned short *>(a.key_scratch);
                hipLaunchKernelGGL((k_predict_keys16<T, V>), dim3(div_up((long long)g.batch * ns, kBlock)), dim3(kBlock), 0, a.st, c, v, g, ns, keys16);
                hipLaunchKernelGGL((k_predict_select_reg<T, 36, false, V>), frames, wg, 0, a.st, c, v, g, a.k, a.score_thr, keys16, ns, a.top_idx,
                                   a.top_score, a.top_label, a.counts, 0, (const int *)nullptr, thr16);
            } else {
                // The candidate arrays live in key_scratch: n2 = chunks * 1024 slots per frame, 4 bytes of anchor id then 2 bytes of key
                // each, inside the 4 bytes per anchor the caller provides.  They always fit: both chunked forms have c >= 2 chunks of
                // P = 8192 or 73 728 anchors, so a frame has more than (c - 1) P anchors, and 6144 c <= 4 ((c - 1) P + 1) holds for every
                // c >= 2 at either P (at c = 2 and P = 8192: 12 288 <= 32 772; the right side grows faster in c).
                const int n2 = plan.chunks * kSelThreads;
                int *ci = reinterpret_cast<int *>(a.key_scratch);
                unsigned short *ck = reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(a.key_scratch) + (size_t)g.batch * n2 * 4);
                auto stage1 = [&](auto kp) {
                    hipLaunchKernelGGL((k_predict_select_chunk<T, decltype(kp)::value, V>), dim3(plan.chunks, g.batch), wg, 0, a.st, c, v, g,
                                       (int)nfr, a.k, plan.chunks, thr16, ck, ci);
                };
                auto stage2 = [&](auto kp2) {
                    hipLaunchKernelGGL((k_predict_select_reg<T, decltype(kp2)::value, true, V>), frames, wg, 0, a.st, c, v, g, a.k, a.score_thr, ck,
                                       n2, a.top_idx, a.top_score, a.top_label, a.counts, n2, ci, thr16);
                };
                plan.kp == 4 ? stage1(Int<4>{}) : stage1(Int<36>{});
                plan.kp2 == 5 ? stage2(Int<5>{}) : plan.kp2 == 10 ? stage2(Int<10>{}) : plan.kp2 == 20 ? stage2(Int<20>{}) : stage2(Int<36>{});
            }
        }
        return check_launch();
    });
}

// the select over one head tensor of any form
static int predict_select_head(const void *cls, const int64_t *h_cls_strides5, const PredGeom &g, const SelectArgs &a, const HeadForm &f) {
    if (!a.key_scratch) return SEC_E_WORKSPACE;
    if (!cls || !h_cls_strides5 || g.batch <= 0 || g.A <= 0 || g.H <= 0 || g.W <= 0 || g.nc <= 0 || a.k <= 0 || a.k > kSelThreads || !a.top_idx ||
        !a.top_score || !a.top_label || !a.counts || !dtype_ok(a.dtype))
        return SEC_E_INVALID;
    View5 v;
    if (int rc = head_view(f, h_cls_strides5, cls, f.background, g.H, g.W, a.dtype, &v)) return rc;
    // a masked-out anchor's key stands for no score; with a threshold <= 0 (no shipped config has one) it would be counted
    if (f.anchor_mask && !(a.score_thr > 0.0f)) return SEC_E_UNSUPPORTED;
    return predict_select_launch(cls, v, g, a);
}

SEC_API int sec_predict_select(const void *cls, const int64_t *h_cls_strides5, int batch, int anchors_per_loc, int h, int w,
                               int num_class, int k, float score_thr, unsigned *key_scratch, int *top_idx, float *top_score,
                               int *top_label, int *counts, int dtype, void *stream) {
    return predict_select_head(cls, h_cls_strides5, {batch, anchors_per_loc, h, w, num_class},
                               {k, score_thr, key_scratch, top_idx, top_score, top_label, counts, dtype, (hipStream_t)stream}, HeadForm{});
}
SEC_API int sec_predict_select_lazy(const void *cls, const int64_t *h_cls_strides5, int batch, int anchors_per_loc, int h, int w,
                                    int num_class, int k, float score_thr, unsigned *key_scratch, int *top_idx, float *top_score,
                                    int *top_label, int *counts, int dtype, const unsigned short *tile_live, const void *cls_background,
                                    void *stream) {
    if (!tile_live || !cls_background) return SEC_E_INVALID;
    return predict_select_head(cls, h_cls_strides5, {batch, anchors_per_loc, h, w, num_class},
                               {k, score_thr, key_scratch, top_idx, top_score, top_label, counts, dtype, (hipStream_t)stream},
                               {tile_live, nullptr, cls_background, nullptr, nullptr});
}
// sec_predict_select / _lazy with the anchor-area mask of sec_anchor_area_mask: frame b keeps the anchors with anchor_mask[b][n] != 0
// (voxelnet.py:429-439 indexes the frame's head rows by the mask before the score threshold); indices stay indices into the full
// anchor list.  tile_live / cls_background both NULL (eager heads) or both set (lazy heads); anchor_mask NULL: exactly those two.
SEC_API int sec_predict_select_masked(const void *cls, const int64_t *h_cls_strides5, int batch, int anchors_per_loc, int h, int w,
                                      int num_class, int k, float score_thr, unsigned *key_scratch, int *top_idx, float *top_score,
                                      int *top_label, int *counts, int dtype, const unsigned short *tile_live, const void *cls_background,
                                      const unsigned char *anchor_mask, void *stream) {
    return predict_select_head(cls, h_cls_strides5, {batch, anchors_per_loc, h, w, num_class},
                               {k, score_thr, key_scratch, top_idx, top_score, top_label, counts, dtype, (hipStream_t)stream},
                               {tile_live, nullptr, cls_background, nullptr, anchor_mask});
}
// The lazy heads behind a COVER-form producer (sec_conv2d_nhwc_tiles_tail_cover): an element was written when bit x of
// cover_cols[b][y >> 3] is set (the last conv's coverage masks of sec_rpn_tile_cover, [B][ceil(h / 8)][ceil(w / 32)] words); every other
// element is read from the empty frame's map.  anchor_mask may be NULL (sec_predict_select_masked otherwise).
SEC_API int sec_predict_select_cover(const void *cls, const int64_t *h_cls_strides5, int batch, int anchors_per_loc, int h, int w,
                                     int num_class, int k, float score_thr, unsigned *key_scratch, int *top_idx, float *top_score,
                                     int *top_label, int *counts, int dtype, const unsigned *cover_cols, const void *cls_background,
                                     const unsigned char *anchor_mask, void *stream) {
    if (!cover_cols || !cls_background) return SEC_E_INVALID;
    return predict_select_head(cls, h_cls_strides5, {batch, anchors_per_loc, h, w, num_class},
                               {k, score_thr, key_scratch, top_idx, top_score, top_label, counts, dtype, (hipStream_t)stream},
                               {nullptr, cover_cols, cls_background, nullptr, anchor_mask});
}

// ---- decode -------------------------------------------------------------------------------------------------------------------
struct DecodeArgs {                                  // what every decode entry point takes besides its head(s)
    int num_dir_bins, k; const float *anchors; const int *top_idx; const float *top_score; int rotate; float *decoded, *dets; int *dir_label;
    int dtype; hipStream_t st;
    int box_ndim = 7;                                // values per box row: 7 + custom_ndim (the _nd entry points), else 7
};
constexpr int kBoxMaxNdim = SEC_BOX_MAX_NDIM;
static bool box_ndim_ok(int nd) { return nd >= 7 && nd <= kBoxMaxNdim; }
// the decode of a validated call; V as in predict_select_launch.  `dir` of the kernel says whether there is a direction head (with
// a SegView that is all it says: the addresses come from vb / vd)
template <typename V>
static int predict_decode_launch(const void *box, const V &vb, const void *dir, const V &vd, const PredGeom &g, const DecodeArgs &a) {
    return by_dtype(a.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const dim3 grid(div_up((long long)g.batch * a.k, kBlock));
        if (a.box_ndim == 7)                         // seven values: the kernel of the entry points without a width
            hipLaunchKernelGGL((k_predict_decode<T, V>), grid, dim3(kBlock), 0, a.st, (const T *)box, vb,
                               (const T *)dir, vd, a.num_dir_bins, g, a.k, a.anchors, a.top_idx, a.top_score, a.rotate, a.decoded, a.dets, a.dir_label);
        else
            hipLaunchKernelGGL((k_predict_decode_nd<T, V>), grid, dim3(kBlock), 0, a.st, (const T *)box, vb,
                               (const T *)dir, vd, a.num_dir_bins, g, a.k, a.anchors, a.top_idx, a.top_score, a.rotate, a.decoded, a.dets, a.dir_label,
                               a.box_ndim);
        return check_launch();
    });
}

// the decode over one head tensor of any form (g.nc unused)
static int predict_decode_head(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5, const PredGeom &g,
                               const DecodeArgs &a, const HeadForm &f) {
    if (!box || !h_box_strides5 || g.batch <= 0 || a.k <= 0 || !a.anchors || !a.top_idx || !a.top_score || !a.decoded || !a.dets || !a.dir_label ||
        !dtype_ok(a.dtype))
        return SEC_E_INVALID;
    if (!box_ndim_ok(a.box_ndim)) return SEC_E_UNSUPPORTED;
    View5 vb, vd{};
    int rc = head_view(f, h_box_strides5, box, f.background, g.H, g.W, a.dtype, &vb);
    if (!rc && dir) rc = head_view(f, h_dir_strides5, dir, f.dir_background, g.H, g.W, a.dtype, &vd);
    return rc ? rc : predict_decode_launch(box, vb, dir, vd, g, a);
}

SEC_API int sec_predict_decode(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5,
                               int num_dir_bins, int batch, int anchors_per_loc, int h, int w, int k, const float *anchors,
                               const int *top_idx, const float *top_score, int rotate, float *decoded, float *dets,
                               int *dir_label, int dtype, void *stream) {
    return predict_decode_head(box, h_box_strides5, dir, h_dir_strides5, {batch, anchors_per_loc, h, w, 1},
                               {num_dir_bins, k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream}, HeadForm{});
}
SEC_API int sec_predict_decode_lazy(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5,
                                    int num_dir_bins, int batch, int anchors_per_loc, int h, int w, int k, const float *anchors,
                                    const int *top_idx, const float *top_score, int rotate, float *decoded, float *dets,
                                    int *dir_label, int dtype, const unsigned short *tile_live, const void *box_background,
                                    const void *dir_background, void *stream) {
    if (!tile_live || !box_background) return SEC_E_INVALID;
    return predict_decode_head(box, h_box_strides5, dir, h_dir_strides5, {batch, anchors_per_loc, h, w, 1},
                               {num_dir_bins, k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream},
                               {tile_live, nullptr, box_background, dir_background, nullptr});
}
SEC_API int sec_predict_decode_cover(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5,
                                     int num_dir_bins, int batch, int anchors_per_loc, int h, int w, int k, const float *anchors,
                                     const int *top_idx, const float *top_score, int rotate, float *decoded, float *dets,
                                     int *dir_label, int dtype, const unsigned *cover_cols, const void *box_background,
                                     const void *dir_background, void *stream) {
    if (!cover_cols || !box_background) return SEC_E_INVALID;
    return predict_decode_head(box, h_box_strides5, dir, h_dir_strides5, {batch, anchors_per_loc, h, w, 1},
                               {num_dir_bins, k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream},
                               {nullptr, cover_cols, box_background, dir_background, nullptr});
}

// sec_predict_decode with rows of box_ndim values; the head's form is given by its tables (at most one of tile_live / cover_cols)
SEC_API int sec_predict_decode_nd(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5,
                                  int num_dir_bins, int batch, int anchors_per_loc, int h, int w, int k, const float *anchors,
                                  const int *top_idx, const float *top_score, int rotate, float *decoded, float *dets,
                                  int *dir_label, int dtype, int box_ndim, const unsigned short *tile_live, const unsigned *cover_cols,
                                  const void *box_background, const void *dir_background, void *stream) {
    return predict_decode_head(box, h_box_strides5, dir, h_dir_strides5, {batch, anchors_per_loc, h, w, 1},
                               {num_dir_bins, k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream, box_ndim},
                               {tile_live, cover_cols, box_background, dir_background, nullptr});
}

static int predict_finalize_impl(const float *decoded, const float *top_score, const int *top_label, const int *dir_label,
                                 const int *keep, const int *num_keep, int batch, int k, int post_max, int use_direction,
                                 float dir_offset, float dir_limit_offset, int num_dir_bins, const float *range6,
                                 float *boxes, float *scores, int *labels, unsigned char *valid, int box_ndim, void *stream) {
    if (!decoded || !top_score || !top_label || !keep || !num_keep || batch <= 0 || k <= 0 || post_max <= 0 || post_max > k ||
        !boxes || !scores || !labels || !valid || (use_direction && (!dir_label || num_dir_bins <= 0)))
        return SEC_E_INVALID;
    if (!box_ndim_ok(box_ndim)) return SEC_E_UNSUPPORTED;
    float period = use_direction ? 6.283185307179586f / (float)num_dir_bins : 0.0f;
    const dim3 grid(div_up((long long)batch * post_max, kBlock));
    if (box_ndim == 7)
        hipLaunchKernelGGL(k_predict_finalize, grid, dim3(kBlock), 0, (hipStream_t)stream,
                           decoded, top_score, top_label, dir_label, keep, num_keep, batch, k, post_max, use_direction, dir_offset,
                           dir_limit_offset, period, range6, boxes, scores, labels, valid);
    else
        hipLaunchKernelGGL(k_predict_finalize_nd, grid, dim3(kBlock), 0, (hipStream_t)stream,
                           decoded, top_score, top_label, dir_label, keep, num_keep, batch, k, post_max, use_direction, dir_offset,
                           dir_limit_offset, period, range6, boxes, scores, labels, valid, box_ndim);
    return check_launch();
}
SEC_API int sec_predict_finalize(const float *decoded, const float *top_score, const int *top_label, const int *dir_label,
                                 const int *keep, const int *num_keep, int batch, int k, int post_max, int use_direction,
                                 float dir_offset, float dir_limit_offset, int num_dir_bins, const float *range6,
                                 float *boxes, float *scores, int *labels, unsigned char *valid, void *stream) {
    return predict_finalize_impl(decoded, top_score, top_label, dir_label, keep, num_keep, batch, k, post_max, use_direction, dir_offset,
                                 dir_limit_offset, num_dir_bins, range6, boxes, scores, labels, valid, 7, stream);
}
SEC_API int sec_predict_finalize_nd(const float *decoded, const float *top_score, const int *top_label, const int *dir_label,
                                    const int *keep, const int *num_keep, int batch, int k, int post_max, int use_direction,
                                    float dir_offset, float dir_limit_offset, int num_dir_bins, const float *range6,
                                    float *boxes, float *scores, int *labels, unsigned char *valid, int box_ndim, void *stream) {
    return predict_finalize_impl(decoded, top_score, top_label, dir_label, keep, num_keep, batch, k, post_max, use_direction, dir_offset,
                                 dir_limit_offset, num_dir_bins, range6, boxes, scores, labels, valid, box_ndim, stream);
}

// ---- several head tensors ---------------------------------------------------------------------------------------------------
// strides5 [S][5] = {sb, sa, sy, sx, sc} and dims3 [S][3] = {A_s, H_s, W_s} are host arrays; the segment pointers are device pointers
static int mksegs(int num_segments, const void *const *ptrs, const int64_t *strides5, const int *dims3, SegView *out, long long *total) {
    if (num_segments < 1 || num_segments > kMaxSegments || !ptrs || !strides5 || !dims3) return SEC_E_INVALID;
    long long n = 0;
    Seg g[kMaxSegments];
    for (int s = 0; s < kMaxSegments; ++s) {
        const int j = s < num_segments ? s : 0;                 // unused entries repeat segment 0 and are never selected
        if (!ptrs[j] || dims3[3 * j] <= 0 || dims3[3 * j + 1] <= 0 || dims3[3 * j + 2] <= 0) return SEC_E_INVALID;
        g[s] = Seg{ptrs[j], strides5[5 * j], strides5[5 * j + 1], strides5[5 * j + 2], strides5[5 * j + 3], strides5[5 * j + 4],
                   dims3[3 * j + 1], dims3[3 * j + 2], (int)n};       // (start = the total for the unused entries)
        if (s < num_segments) n += (long long)dims3[3 * j] * dims3[3 * j + 1] * dims3[3 * j + 2];
        if (n > 0x7fffffffll) return SEC_E_UNSUPPORTED;
    }
    SegView v{g[0], g[1], g[2], g[3], (int)n};
    *out = v;
    *total = n;
    return SEC_OK;
}

SEC_API int sec_predict_select_segments(int num_segments, const void *const *cls, const int64_t *h_cls_strides5, const int *h_dims3,
                                        int batch, int num_class, int k, float score_thr, unsigned *key_scratch, int *top_idx,
                                        float *top_score, int *top_label, int *counts, int dtype, void *stream) {
    SegView v;
    long long n;
    if (int rc = mksegs(num_segments, cls, h_cls_strides5, h_dims3, &v, &n)) return rc;
    if (k > kSelThreads) return SEC_E_UNSUPPORTED;
    if (batch <= 0 || num_class <= 0 || k <= 0 || !top_idx || !top_score || !top_label || !counts || !dtype_ok(dtype)) return SEC_E_INVALID;
    if ((long long)batch * n > 0x7fffffffll) return SEC_E_UNSUPPORTED;
    if (!key_scratch) return SEC_E_WORKSPACE;
    // the kernels take N = A * H * W from the geometry; addresses come from the segments
    return predict_select_launch((const void *)nullptr, v, PredGeom{batch, 1, 1, (int)n, num_class},
                                 {k, score_thr, key_scratch, top_idx, top_score, top_label, counts, dtype, (hipStream_t)stream});
}

static int predict_decode_segments_impl(int num_segments, const void *const *box, const int64_t *h_box_strides5, const void *const *dir,
                                        const int64_t *h_dir_strides5, const int *h_dims3, int num_dir_bins, int batch, int k,
                                        const float *anchors, const int *top_idx, const float *top_score, int rotate, float *decoded,
                                        float *dets, int *dir_label, int dtype, int box_ndim, void *stream) {
    SegView vb{}, vd{};
    long long n;
    if (int rc = mksegs(num_segments, box, h_box_strides5, h_dims3, &vb, &n)) return rc;
    if (dir)
        if (int rc = mksegs(num_segments, dir, h_dir_strides5, h_dims3, &vd, &n)) return rc;
    if (k > kSelThreads) return SEC_E_UNSUPPORTED;
    if (batch <= 0 || k <= 0 || !anchors || !top_idx || !top_score || !decoded || !dets || !dir_label || !dtype_ok(dtype) ||
        (dir && num_dir_bins <= 0))
        return SEC_E_INVALID;
    if (!box_ndim_ok(box_ndim)) return SEC_E_UNSUPPORTED;
    return predict_decode_launch((const void *)nullptr, vb, dir ? dir[0] : nullptr, vd, PredGeom{batch, 1, 1, (int)n, 1},
                                 {num_dir_bins, k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream, box_ndim});
}
SEC_API int sec_predict_decode_segments(int num_segments, const void *const *box, const int64_t *h_box_strides5, const void *const *dir,
                                        const int64_t *h_dir_strides5, const int *h_dims3, int num_dir_bins, int batch, int k,
                                        const float *anchors, const int *top_idx, const float *top_score, int rotate, float *decoded,
                                        float *dets, int *dir_label, int dtype, void *stream) {
    return predict_decode_segments_impl(num_segments, box, h_box_strides5, dir, h_dir_strides5, h_dims3, num_dir_bins, batch, k, anchors, top_idx,
                                        top_score, rotate, decoded, dets, dir_label, dtype, 7, stream);
}
SEC_API int sec_predict_decode_segments_nd(int num_segments, const void *const *box, const int64_t *h_box_strides5, const void *const *dir,
                                           const int64_t *h_dir_strides5, const int *h_dims3, int num_dir_bins, int batch, int k,
                                           const float *anchors, const int *top_idx, const float *top_score, int rotate, float *decoded,
                                           float *dets, int *dir_label, int dtype, int box_ndim, void *stream) {
    return predict_decode_segments_impl(num_segments, box, h_box_strides5, dir, h_dir_strides5, h_dims3, num_dir_bins, batch, k, anchors, top_idx,
                                        top_score, rotate, decoded, dets, dir_label, dtype, box_ndim, stream);
}

// ---- multi-class NMS: (frame, class) items -----------------------------------------------------------------------------------
SEC_API int sec_predict_select_classes(const void *cls, const int64_t *h_cls_strides5, int batch, int anchors_per_loc, int h, int w,
                                       int num_class, const int *h_a_begin, const int *h_a_end, const int *h_k, const float *h_score_thr,
                                       int k_out, int *top_idx, float *top_score, int *counts, int dtype,
                                       const unsigned char *anchor_mask, void *stream) {
    if (!cls || !h_cls_strides5 || batch <= 0 || anchors_per_loc <= 0 || h <= 0 || w <= 0 || num_class <= 0 || !h_a_begin || !h_a_end ||
        !h_k || !h_score_thr || k_out <= 0 || k_out > kSelThreads || !top_idx || !top_score || !counts || !dtype_ok(dtype))
        return SEC_E_INVALID;
    if (anchor_mask) return SEC_E_UNSUPPORTED;            // the reference indexes masked arrays with unmasked ranges here: not reproduced
    if (num_class > kMaxSelClasses) return SEC_E_UNSUPPORTED;
    if ((long long)anchors_per_loc * h * w > 0x7fffffffll || (long long)batch * num_class * k_out > 0x7fffffffll) return SEC_E_UNSUPPORTED;
    ClassSel p{};
    for (int c = 0; c < num_class; ++c) {
        if (h_a_begin[c] < 0 || h_a_end[c] > anchors_per_loc || h_a_begin[c] >= h_a_end[c] || h_k[c] <= 0) return SEC_E_INVALID;
        if (h_k[c] > kSelThreads) return SEC_E_UNSUPPORTED;                   // the caller takes the torch.topk formulation
        if (!(h_score_thr[c] > 0.0f)) return SEC_E_UNSUPPORTED;               // a key of 0 stands for "no candidate"
        const long long n = (long long)(h_a_end[c] - h_a_begin[c]) * h * w;
        if ((n < h_k[c] ? n : (long long)h_k[c]) > k_out) return SEC_E_INVALID;   // the item's rows do not fit [B, C, k_out]
        p.a_begin[c] = h_a_begin[c]; p.a_end[c] = h_a_end[c]; p.k[c] = h_k[c]; p.thr[c] = h_score_thr[c];
    }
    const PredGeom g{batch, anchors_per_loc, h, w, num_class};
    const View5 v = mkview(h_cls_strides5);
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_predict_select_classes<T>, dim3(num_class, batch), dim3(kSelThreads), 0, (hipStream_t)stream, (const T *)cls, v, g,
                           p, k_out, top_idx, top_score, counts);
        return check_launch();
    });
}

// the rows of all items are one list of num_class * k rows per frame: sec_predict_decode's kernel on [B, num_class * k]
SEC_API int sec_predict_decode_classes(const void *box, const int64_t *h_box_strides5, const void *dir, const int64_t *h_dir_strides5,
                                       int num_dir_bins, int batch, int anchors_per_loc, int h, int w, int num_class, int k,
                                       const float *anchors, const int *top_idx, const float *top_score, int rotate, float *decoded,
                                       float *dets, int *dir_label, int dtype, void *stream) {
    if (num_class <= 0 || k <= 0 || (long long)batch * num_class * k > 0x7fffffffll / 7) return SEC_E_INVALID;
    return predict_decode_head(box, h_box_strides5, dir, h_dir_strides5, {batch, anchors_per_loc, h, w, 1},
                               {num_dir_bins, num_class * k, anchors, top_idx, top_score, rotate, decoded, dets, dir_label, dtype, (hipStream_t)stream},
                               HeadForm{});
}

SEC_API int sec_predict_finalize_classes(const float *decoded, const float *top_score, const int *dir_label, const int *keep,
                                         const int *num_keep, const int *post_offsets, int batch, int num_class, int k, int post_total,
                                         int use_direction, float dir_offset, float dir_limit_offset, int num_dir_bins,
                                         const float *range6, float *boxes, float *scores, int *labels, unsigned char *valid,
                                         void *stream) {
    if (!decoded || !top_score || !keep || !num_keep || !post_offsets || batch <= 0 || num_class <= 0 || k <= 0 || post_total <= 0 ||
        (long long)batch * post_total > 0x7fffffffll / 7 || !boxes || !scores || !labels || !valid ||
        (use_direction && (!dir_label || num_dir_bins <= 0)))
        return SEC_E_INVALID;
    float period = use_direction ? 6.283185307179586f / (float)num_dir_bins : 0.0f;
    hipLaunchKernelGGL(k_predict_finalize_classes, dim3(div_up((long long)batch * post_total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       decoded, top_score, dir_label, keep, num_keep, post_offsets, batch, num_class, k, post_total, use_direction, dir_offset,
                       dir_limit_offset, period, range6, boxes, scores, labels, valid);
    return check_launch();
}
