// fp32 convolutions of the single-block RPN on the matrix pipe's fp32 instruction (v_mfma_f32_32x32x2_f32): the exact-precision
// counterpart of k_conv2d_halo_reg<..., X3> / k_conv1x1_chain_x3 in dense.hip.  fp32 channels-last images [B][H][W][C], fp32
// weights, fp32 accumulation, bias + ReLU in the epilogue, fp32 output -- every output element is ONE fma chain over
// k = (tap, input channel) in a fixed order that does not depend on the call form, the tile or the lane:
//     for tap in 0..8: for kq in 0..15: for j in 0..3: acc = fma(x[kq*8 + j], w[kq*8 + j], acc); acc = fma(x[kq*8 + 4 + j], w[kq*8 + 4 + j], acc)
// (the instruction's two k values are channels c and c + 4, so that a lane's four k-steps are ONE 16-byte LDS read and ONE 16-byte
// weight load).  That fixed order is what makes a tile of the list forms bit-identical to the same tile of the full form, and the
// copied / lazily read background tiles exact for any weights.
//
// 3x3 kernel: the same 8 x 16 pixel tiles, tile lists, neighbour masks and XCD-contiguous order as k_conv2d_halo_reg.  The fp32 halo
// of a tile is 10 * 18 * 128 * 4 = 92 160 B of LDS (one workgroup per CU), fetched by buffer LDS-DMA whose bounds check supplies the
// zero padding; a wave owns all 128 pixels for 32 output channels = four independent 32 x 32 accumulators, which is what the fp32 MFMA
// needs to issue back to back.  At 1/16 of the bf16 rate the loop is matrix bound (144 iterations x 16 MFMAs x 64 clocks per wave
// against one 1 KB weight load and four LDS reads per iteration), so weights are streamed from L2 two iterations ahead and halo
// fragments one iteration ahead, nothing more.
#include "common.hpp"

namespace sec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void *lds_ptr_t;

constexpr int kTH = 8, kTW = 16, kHW = kTW + 2, kHPix = (kTH + 2) * kHW;    // tile, halo width, halo pixels
constexpr int kCh = 32;                                                       // 16-byte chunks of a 128-channel fp32 pixel
constexpr size_t kConvLds = (size_t)kHPix * kCh * 16;                         // 92 160 B
constexpr size_t kChainLds = (size_t)128 * kCh * 16;                          // 65 536 B: 128 pixels
constexpr int kCopyTiles = 4;                                                 // background tiles per copying workgroup

// torch [cout][128][ks][ks] -> [tap][kq = 16][cout / 32][lane = 64] float4: lane l holds, for its output channel nb * 32 + (l & 31),
// the input channels kq * 8 + (l >> 5) * 4 + {0, 1, 2, 3} -- k-step j of the MFMA loop takes component j, i.e. B[k = l >> 5][col = l & 31]
__global__ __launch_bounds__(kBlock) void k_conv2d_pack_f32(const float *__restrict__ w, int cout, int ks, float4 *__restrict__ packed, long long total) {
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    long long t = idx >> 6;
    const int nbk = cout / 32;
    const int nb = (int)(t % nbk); t /= nbk;
    const int kq = (int)(t % 16);
    const int tap = (int)(t / 16);
    const int co = nb * 32 + (lane & 31), ci = kq * 8 + (lane >> 5) * 4;
    const int kk = ks * ks;
    const float *src = w + ((size_t)co * 128 + ci) * kk + tap;
    packed[idx] = make_float4(src[0], src[kk], src[2 * kk], src[3 * kk]);
}

// acc[mt] += W[32 channels of this wave][K] * X[K][32 pixels of m-tile mt] over NTAP taps x 128 input channels.  `hal` = pixels of 32
// swizzled 16-byte chunks (chunk c of pixel p at p * 32 + (c ^ key(p))); pixel of lane / m-tile = hp0[mt] (+ dy * 18 + dx per tap),
// key = (hx0[mt] + dx) & 15: the 16 lanes one ds_read_b128 serves together are 16 consecutive columns, so their keys -- and with
// them their 16-byte slots of the 256-byte bank row -- are distinct.
template <int MT, int NTAP>
__device__ __forceinline__ void gemm_f32(f32x16 (&acc)[MT], const uint4 *hal, const int (&hp0)[MT], const int (&hx0)[MT], int hh,
                                         __amdgpu_buffer_rsrc_t wrs, unsigned wvoff, unsigned wstep) {
    float4 bq[4];
    uint4 ac[MT], an[MT];
    int base[MT], key[MT];
    auto ldb = [&](int it) {     // past the last iteration: out of the resource's bounds, returns zeros that nobody uses
        return __builtin_bit_cast(float4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(wrs, wvoff, (unsigned)it * wstep, 0));
    };
    auto set_tap = [&](int tap, int (&b_)[MT], int (&k_)[MT]) {
        const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            b_[mt] = (hp0[mt] + dy * kHW + dx) * kCh;
            k_[mt] = (hx0[mt] + dx) & 15;
        }
    };
    auto lda = [&](int kq, const int (&b_)[MT], const int (&k_)[MT], uint4 (&dst)[MT]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) dst[mt] = hal[b_[mt] + ((kq * 2 + hh) ^ k_[mt])];
    };
    bq[0] = ldb(0);
    bq[1] = ldb(1);
    set_tap(0, base, key);
    lda(0, base, key, ac);
#pragma unroll 1
    for (int tap = 0; tap < NTAP; ++tap) {
        int nbase[MT], nkey[MT];
        set_tap(tap + 1 < NTAP ? tap + 1 : tap, nbase, nkey);
#pragma unroll
        for (int kq = 0; kq < 16; ++kq) {
            bq[(kq + 2) & 3] = ldb(tap * 16 + kq + 2);
            if (kq < 15) lda(kq + 1, base, key, an);
            else lda(0, nbase, nkey, an);
            // the scheduler otherwise sinks these loads to just above their first use (next iteration) and the wave waits out the
            // LDS / L2 latency there: keep them above this iteration's sixteen MFMAs
            __builtin_amdgcn_sched_barrier(0);
            const float4 b = bq[kq & 3];
            const float bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const unsigned au = j == 0 ? ac[mt].x : (j == 1 ? ac[mt].y : (j == 2 ? ac[mt].z : ac[mt].w));
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bs[j], __builtin_bit_cast(float, au), acc[mt], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ac[mt] = an[mt];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { base[mt] = nbase[mt]; key[mt] = nkey[mt]; }
    }
}

// D[channel][pixel] of the MFMA: a lane holds pixel l & 31 and channels 8 * (i / 4) + 4 * (l >> 5) + i % 4 -- group g = i / 4 is four
// consecutive channels = one float4
__device__ __forceinline__ float4 epilogue4(const f32x16 &a, int g, const float *__restrict__ bias, int c, int relu) {
    float v[4] = {a[g * 4], a[g * 4 + 1], a[g * 4 + 2], a[g * 4 + 3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = v[j] + (bias ? bias[c + j] : 0.0f);
        if (relu) v[j] = __builtin_fmaxf(v[j], 0.0f);
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// One kernel, three call forms (sec_conv2d_nhwc_f32 / sec_conv2d_nhwc_f32_tiles):
//   tile_order == NULL: every tile; zskip: a tile whose halo is all zero bits skips the MFMA loop (its accumulators would be +0);
//   tile_order + background: the live tiles of the lists are convolved, the others copied from `background` [h][w][cout];
//   tile_order, no background (lazy): only live tiles are written; nbr_masks (rank-indexed half) says which of the nine tiles around
//   a live tile the producer of `x` wrote -- halo pixels of the others are read from `bg_in`, the producer's empty-frame map.
// The lists are honoured whatever the live share: the loop is long enough that the list lookups never show.
__global__ __launch_bounds__(256) void k_conv2d_f32(const float *__restrict__ x, const float *__restrict__ wpk, const float *__restrict__ bias,
                                                    float *__restrict__ y, int batch, int h, int w, int cout, int relu, int zskip,
                                                    int tiles_y, int tiles_x, int per_xcd, const unsigned short *__restrict__ tile_order,
                                                    const int *__restrict__ live_counts, const float *__restrict__ background,
                                                    const unsigned short *__restrict__ nbr_masks, const float *__restrict__ bg_in) {
    // A workgroup computes 128 output channels, a wave all 128 pixels x 32 of them (four accumulators).  Measured against it: 64 channels
    // per workgroup (a wave 64 pixels x 32 channels, two accumulators; twice the workgroups of half the length, meant to shorten the
    // last round when ~700 live tiles meet 256 CUs) -- 294 instead of 253 us on 728 live tiles, 808 instead of 760 us on all 2200: every
    // workgroup pays the whole 92 KB halo and, alone on its CU, nothing hides that prologue.
    constexpr int MT = 4, kC4 = 32;
    extern __shared__ __attribute__((aligned(16))) uint4 halo_f32[];
    uint4 *hal = halo_f32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int tpf = tiles_y * tiles_x, ntile = batch * tpf;
    const int xcd = blockIdx.x % 8, local = blockIdx.x / 8;      // workgroup b runs on XCD b % 8: contiguous tile ranges per XCD
    if (local >= per_xcd) return;
    int tile = xcd * per_xcd + local;
    unsigned nmask = 0x1ffu;
    if (tile_order) {
        int n_live = 0;
        for (int f = 0; f < batch; ++f) n_live += live_counts[f];
        const int per_live = (n_live + 7) >> 3;
        int item;
        bool is_live = false;
        if (local < per_live) {
            item = xcd * per_live + local;
            is_live = item < n_live;
            if (!is_live) item -= n_live;
        } else {
            item = 8 * per_live - n_live + (local - per_live) * 8 + xcd;
        }
        if (is_live) {
            int f = 0;
            while (item >= live_counts[f]) item -= live_counts[f++];
            tile = f * tpf + tile_order[f * tpf + item];
            if (nbr_masks) nmask = nbr_masks[f * tpf + item];
        } else {
            if (!background) return;
            // background tiles: the tail of each frame's order, copied from the empty frame's map (this workgroup's 128 channels)
            const int n_bg = ntile - n_live;
            const float4 *e4 = reinterpret_cast<const float4 *>(background);
            float4 *y4 = reinterpret_cast<float4 *>(y);
            const int c4n = cout / 4;
#pragma unroll 1
            for (int q = 0; q < kCopyTiles; ++q) {
                int it = item * kCopyTiles + q;
                if (it >= n_bg) break;
                int f = 0;
                while (it >= tpf - live_counts[f]) it -= tpf - live_counts[f++];
                const int trem = tile_order[f * tpf + tpf - 1 - it];
                const int y0 = (trem / tiles_x) * kTH, x0 = (trem % tiles_x) * kTW;
#pragma unroll 4
                for (int e = tid; e < kTH * kTW * kC4; e += 256) {
                    const int px = e / kC4, c4 = e % kC4;
                    const int oy = y0 + (px >> 4), ox = x0 + (px & 15);
                    if (oy < h && ox < w) {
                        const size_t o = ((size_t)oy * w + ox) * c4n + blockIdx.y * kC4 + c4;
                        y4[(size_t)f * h * w * c4n + o] = e4[o];
                    }
                }
            }
            return;
        }
    }
    if (tile >= ntile) return;
    const int b = tile / tpf, trem = tile - b * tpf;
    const int y0 = (trem / tiles_x) * kTH, x0 = (trem % tiles_x) * kTW;
    {
        // halo by buffer LDS-DMA: piece i = 1 KB = halo pixels 2 i and 2 i + 1, lane = LDS slot, source chunk = slot ^ key.  Rows above /
        // below the image fall outside the resource (zero fill), the columns left / right of it are sent there by the select.
        const unsigned img_bytes = (unsigned)h * (unsigned)w * 512u;
        const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x) + (size_t)b * h * w * 128, 0, (int)img_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(nbr_masks ? bg_in : x), 0, (int)img_bytes, 0x00020000);
        const unsigned slot = lane & 31;
        const unsigned row_pitch = (unsigned)w * 512u;
        int hx = wv * 2 + hh, hy = 0;
        unsigned rowoff = (unsigned)((y0 - 1) * w + (x0 - 1)) * 512u;      // may wrap below zero: out of bounds, zero fill
        constexpr int NPIECE = kHPix * kCh / 64;
#pragma unroll
        for (int t = 0; t < (NPIECE + 3) / 4; ++t) {
            const int i = wv + 4 * t;
            if (i < NPIECE) {
                const unsigned key = (slot ^ ((unsigned)hx & 15u)) << 4;
                unsigned off = rowoff + ((unsigned)hx << 9) + key;
                const unsigned ix = (unsigned)(x0 - 1 + hx);
                off = ix < (unsigned)w ? off : 0xfffffff0u;
                const int ry = hy == 0 ? 0 : (hy == kTH + 1 ? 2 : 1), rx = hx == 0 ? 0 : (hx == kHW - 1 ? 2 : 1);
                if ((nmask >> (ry * 3 + rx)) & 1u) __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_ptr_t)&hal[i * 64], 16, off, 0, 0, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(ers, (lds_ptr_t)&hal[i * 64], 16, off, 0, 0, 0);
            }
            hx += 8;
            const bool wrap = hx >= kHW;
            hx = wrap ? hx - kHW : hx;
            hy = wrap ? hy + 1 : hy;
            rowoff = wrap ? rowoff + row_pitch : rowoff;
        }
    }
    f32x16 acc[MT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                // halo landed
    bool live = true;
    if (zskip) {
        unsigned nz = 0;
        for (int e = tid; e < kHPix * kCh; e += 256) {
            const uint4 v = hal[e];
            nz |= v.x | v.y | v.z | v.w;
        }
        live = __syncthreads_or((int)(nz != 0)) != 0;
    }
    const int n0 = blockIdx.y * 128 + wv * 32;      // this wave's 32 output channels
    if (live) {
        int hp0[MT], hx0[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int q = mt * 32 + r;
            hp0[mt] = (q >> 4) * kHW + (q & 15);
            hx0[mt] = q & 15;
        }
        const int nbk = cout / 32;
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(wpk), 0, 9 * 16 * nbk * 1024, 0x00020000);
        gemm_f32<MT, 9>(acc, hal, hp0, hx0, hh, wrs, (unsigned)((n0 / 32) * 64 + lane) * 16u, (unsigned)nbk * 1024u);
    }
    float4 *y4 = reinterpret_cast<float4 *>(y);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = mt * 32 + r;
        const int oy = y0 + (q >> 4), ox = x0 + (q & 15);
        if (oy < h && ox < w) {
            const size_t o = (((size_t)b * h + oy) * w + ox) * (cout / 4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = n0 + g * 8 + hh * 4;
                y4[o + c / 4] = epilogue4(acc[mt], g, bias, c, relu);
            }
        }
    }
}

// y = W2 relu(W1 x + b1) + b2 over 128-pixel tiles of [pixels][128]: the tile (64 KB, swizzled like the halo) is multiplied by W1,
// the biased / rectified result replaces it in LDS, and the second product leaves as fp32.  NT2 = cout2 / 64: with 64 output channels
// the waves split the pixels two ways.
template <int NT2>
__global__ __launch_bounds__(256) void k_conv1x1_chain_f32(const float *__restrict__ x, const float *__restrict__ w1pk, const float *__restrict__ b1,
                                                           const float *__restrict__ w2pk, const float *__restrict__ b2, float *__restrict__ y,
                                                           long long pixels, int relu1) {
    extern __shared__ __attribute__((aligned(16))) uint4 halo_f32[];
    uint4 *hal = halo_f32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const long long base = (long long)blockIdx.x * 128;
    const long long left = pixels - base;
    const int npx = left < 128 ? (int)left : 128;
    {
        const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x) + (size_t)base * 128, 0, npx * 512, 0x00020000);
        const unsigned slot = lane & 31;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int i = wv + 4 * t;
            const unsigned px = (unsigned)(i * 2 + hh);
            const unsigned off = (px << 9) + ((slot ^ (px & 15u)) << 4);    // pixels past the end: out of bounds, zero fill
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_ptr_t)&hal[i * 64], 16, off, 0, 0, 0);
        }
    }
    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int hp0[4], hx0[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) hp0[mt] = hx0[mt] = mt * 32 + r;
    {
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w1pk), 0, 16 * 4 * 1024, 0x00020000);
        gemm_f32<4, 1>(acc, hal, hp0, hx0, hh, wrs, (unsigned)(wv * 64 + lane) * 16u, 4u * 1024u);
    }
    __syncthreads();                                // every wave has read the input tile
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int px = mt * 32 + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = wv * 32 + g * 8 + hh * 4;
            const float4 v = epilogue4(acc[mt], g, b1, c, relu1);
            hal[px * kCh + ((c / 4) ^ (px & 15))] = __builtin_bit_cast(uint4, v);
        }
    }
    __syncthreads();
    float4 *y4 = reinterpret_cast<float4 *>(y);
    const __amdgpu_buffer_rsrc_t wrs2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w2pk), 0, 16 * NT2 * 2 * 1024, 0x00020000);
    if constexpr (NT2 == 2) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
        gemm_f32<4, 1>(acc, hal, hp0, hx0, hh, wrs2, (unsigned)(wv * 64 + lane) * 16u, 4u * 1024u);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int px = mt * 32 + r;
            if (px < npx)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = wv * 32 + g * 8 + hh * 4;
                    y4[(size_t)(base + px) * 32 + c / 4] = epilogue4(acc[mt], g, b2, c, 0);
                }
        }
    } else {
        f32x16 acc2[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc2[a][i] = 0.0f;
        const int nb = wv & 1, half = wv >> 1;
        int hq0[2], hq1[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) hq0[mt] = hq1[mt] = (half * 2 + mt) * 32 + r;
        gemm_f32<2, 1>(acc2, hal, hq0, hq1, hh, wrs2, (unsigned)(nb * 64 + lane) * 16u, 2u * 1024u);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int px = hq0[mt];
            if (px < npx)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = nb * 32 + g * 8 + hh * 4;
                    y4[(size_t)(base + px) * 16 + c / 4] = epilogue4(acc2[mt], g, b2, c, 0);
                }
        }
    }
}

// The kernels need more dynamic LDS than a kernel gets without asking; raised once per process (packing a weight does it, so that the
// first launch inside a stream capture finds it done).
int configure_f32() {
    static int state = -1;
    if (state < 0) {
        bool ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_conv2d_f32), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLds) == hipSuccess;
        ok = ok && hipFuncSetAttribute(reinterpret_cast<const void *>(k_conv1x1_chain_f32<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChainLds) == hipSuccess;
        ok = ok && hipFuncSetAttribute(reinterpret_cast<const void *>(k_conv1x1_chain_f32<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChainLds) == hipSuccess;
        if (!ok) { set_last_error(hipGetLastError()); return SEC_E_LAUNCH; }
        state = 1;
    }
    return SEC_OK;
}

int conv2d_f32_impl(const float *x, int batch, int h, int w, const void *packed, const float *bias, int cout, int relu, int zskip,
                    const unsigned short *tile_order, const int *live_counts, const float *background, const unsigned short *nbr_masks,
                    const float *background_in, float *y, void *stream) {
    if (cout <= 0 || cout % 128 || (long long)h * w * 512 >= (1ll << 31)) return SEC_E_UNSUPPORTED;     // 32-bit buffer offsets per frame
    if (const int rc = configure_f32()) return rc;
    const int ty = div_up(h, kTH), tx = div_up(w, kTW);
    const int per_xcd = div_up((long long)batch * ty * tx, 8);
    set_last_kernel("k_conv2d_f32");
    hipLaunchKernelGGL(k_conv2d_f32, dim3(per_xcd * 8, cout / 128), dim3(256), kConvLds, (hipStream_t)stream, x, (const float *)packed, bias, y,
                       batch, h, w, cout, relu & 1, zskip, ty, tx, per_xcd, tile_order, live_counts, background, nbr_masks, background_in);
    return check_launch();
}

}  // namespace
}  // namespace sec

using namespace sec;

SEC_API size_t sec_conv2d_f32_packed_weight_bytes(int cout, int cin, int ksize) {
    if (cout <= 0 || cout % 64 || cin != 128 || (ksize != 1 && ksize != 3) || (ksize == 3 && cout % 128)) return 0;
    return (size_t)ksize * ksize * 128 * cout * 4;       // no padding block: the halo DMA zero-fills through its buffer bounds
}

SEC_API int sec_conv2d_f32_pack_weight(const float *weight, int cout, int cin, int ksize, void *packed, void *stream) {
    if (!weight || !packed) return SEC_E_INVALID;
    if (sec_conv2d_f32_packed_weight_bytes(cout, cin, ksize) == 0) return SEC_E_UNSUPPORTED;
    if (const int rc = configure_f32()) return rc;
    const long long total = (long long)ksize * ksize * 128 * cout / 4;
    hipLaunchKernelGGL(k_conv2d_pack_f32, dim3(div_up(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, weight, cout, ksize, (float4 *)packed, total);
    return check_launch();
}

SEC_API int sec_conv2d_nhwc_f32(const float *x, int batch, int h, int w, const void *packed, const float *bias, int cout, int relu_flags,
                                float *y, void *stream) {
    if (!x || !packed || !y || batch <= 0 || h <= 0 || w <= 0) return SEC_E_INVALID;
    return conv2d_f32_impl(x, batch, h, w, packed, bias, cout, relu_flags & 1, (relu_flags >> 1) & 1, nullptr, nullptr, nullptr, nullptr, nullptr, y, stream);
}

SEC_API int sec_conv2d_nhwc_f32_tiles(const float *x, int batch, int h, int w, const void *packed, const float *bias, int cout, int relu,
                                      const unsigned short *tile_order, const int *live_counts, const float *background,
                                      const unsigned short *nbr_masks, const float *background_in, float *y, void *stream) {
    if (!x || !packed || !y || !tile_order || !live_counts || batch <= 0 || h <= 0 || w <= 0) return SEC_E_INVALID;
    if (nbr_masks && !background_in) return SEC_E_INVALID;
    return conv2d_f32_impl(x, batch, h, w, packed, bias, cout, relu & 1, 0, tile_order, live_counts, background, nbr_masks, background_in, y, stream);
}

SEC_API int sec_conv1x1_chain_f32(const float *x, long long pixels, const void *packed_w1, const float *bias1, int relu1, const void *packed_w2,
                                  const float *bias2, int cout2, float *y, void *stream) {
    if (!x || !packed_w1 || !packed_w2 || !bias1 || !y || pixels < 0) return SEC_E_INVALID;
    if (cout2 != 64 && cout2 != 128) return SEC_E_UNSUPPORTED;
    if (pixels == 0) return SEC_OK;
    if (pixels > 128ll * 0x7fffffff) return SEC_E_UNSUPPORTED;
    if (const int rc = configure_f32()) return rc;
    const int blocks = (int)div_up(pixels, 128);
    if (cout2 == 64)
        hipLaunchKernelGGL(k_conv1x1_chain_f32<1>, dim3(blocks), dim3(256), kChainLds, (hipStream_t)stream, x, (const float *)packed_w1, bias1,
                           (const float *)packed_w2, bias2, y, pixels, relu1 & 1);
    else
        hipLaunchKernelGGL(k_conv1x1_chain_f32<2>, dim3(blocks), dim3(256), kChainLds, (hipStream_t)stream, x, (const float *)packed_w1, bias1,
                           (const float *)packed_w2, bias2, y, pixels, relu1 & 1);
    return check_launch();
}
