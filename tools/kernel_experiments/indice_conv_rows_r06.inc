// Round-6 experiment on the mid-size 64 -> 64 sparse convs (A/B builds only: -DSEC_CONV_EXPERIMENTS; variant 50, or the automatic
// choice with SEC_CONV_KS=1).  Parity-green under tests/test_gpu_conv_rows.py and SLOWER than the shipped four-wave form on the four
// 23 k-row launches of car.fhd at batch 8 (gpurun r06_u, same build, same box: 11.65 / 13.21 / 13.17 / 13.03 us against 11.94 / 12.25 /
// 12.15 / 12.02 us): three times the waves per SIMD on the same bytes per workgroup buy nothing, i.e. the launch is NOT bound by
// the latency chain of its one wave per SIMD but by what a CU pulls through its L2 -> L1 path (221 KB of weight slices + 128 KB of rows).
// Included by indice_conv.hip inside namespace sec.

// ------------------------------------------------------------------------------------------------------------------
// Row-split kernel with the kernel OFFSETS split over wave groups (round 6; 64 -> 64, 27 offsets).  The four-wave form above gives the
// 23 k-row layers of car.fhd 238 workgroups of 96 rows: ONE wave per SIMD that walks all 27 offsets by itself -- gather, wait, eight
// MFMAs, again -- so nothing hides that wave's latencies, and its launch takes 12 us for 2.2 us of matrix work and 360 KB per CU.
// Here a workgroup is TILES row tiles x G groups of waves: the G waves of a tile share its rows (one staged neighbour table) and
// each walks only ITS windows of three offsets (G = 3: one kernel plane dz each) with its own accumulators, its group's own
// six-slot weight ring and the same counted waits; G waves per SIMD interleave where one sat idle.  At the end groups 1 .. G-1 hand
// their fp32 accumulators to group 0 through LDS (the rings are free by then), which adds them in group order -- a fixed summation
// order, (dz = 0) + (dz = 1) + (dz = 2): deterministic, and no memory traffic the four-wave form does not have (same weight bytes
// per workgroup, same gathers, same LDS reads of B fragments).  Rows per wave (BAL), XCD-contiguous tile order, lazy table reads,
// out-of-range offsets for missing neighbours: as in k_conv_rows_buf.
template <typename T, int TILES, int G, int ABL = 0>   // ABL (timing only, -DSEC_CONV_ABLATIONS): 1 = no gather touches memory, 2 = no weight loads
__global__ __launch_bounds__(TILES * G * 64) void k_conv_rows_ks(const T *__restrict__ feat, long long feat_bytes, const T *__restrict__ packed,
                                                                   const int *__restrict__ nbr, int n_out, const int *__restrict__ num_out_dev,
                                                                   const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                                   T *__restrict__ out) {
    using C = RowsCfg<T, 64, 64>;
    constexpr int KVOL = 27, DIST = 3, NWIN = KVOL / 3;
    constexpr int WMAX = (NWIN + G - 1) / G;             // windows of the largest group (= barriers of the loop)
    constexpr bool EVEN = NWIN % G == 0;
    constexpr int WPW = 24 / TILES;                      // 1 KB weight pieces per wave and window (a window = 3 offsets = 24 pieces)
    static_assert(24 % TILES == 0 && C::BSLOT == 512 && C::KS == 4 && C::NT == 2, "64 -> 64: eight 1 KB pieces per offset");
    constexpr int TBL16 = 32 * KVOL / 4;                 // 16-byte pieces of one tile's neighbour table
    constexpr int PER = (TBL16 + G - 1) / G;             // ... staged by each wave of the tile
    constexpr int WIN16 = 3 * C::BSLOT;                  // uint4 entries of one window of weights
    extern __shared__ __attribute__((aligned(16))) uint4 ks_smem[];
    uint4 *ring = ks_smem;                                                   // [G][2][WIN16]
    u32x4_t *stage = reinterpret_cast<u32x4_t *>(ks_smem + G * 2 * WIN16);   // [TILES][TBL16]
    float *aff = reinterpret_cast<float *>(stage + TILES * TBL16);           // scale[64] | shift[64]
    rows_stage_affine<64>(aff, scale, shift);
    const int n_cap = n_out;
    if (num_out_dev) n_out = *num_out_dev;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int t = w % TILES, g = w / TILES;
    const int r = lane & 31, h = lane >> 5;
    int rw;
    {
        const int per_wg = (n_out + kBalWgs - 1) / kBalWgs;
        rw = ((per_wg + TILES - 1) / TILES + 3) & ~3;
        rw = rw < 4 ? 4 : (rw > 32 ? 32 : rw);
    }
    int bid = blockIdx.x;
    if (relu & 0x10000) {                                // XCD-contiguous tile order (see k_conv_rows_buf)
        const int nact = (int)(((long long)n_out + rw * TILES - 1) / (rw * TILES));
        const int per = (nact + 7) >> 3;
        bid = (bid & 7) * per + (bid >> 3);
        if ((int)(blockIdx.x >> 3) >= per) return;
    }
    relu &= 1;
    if ((long long)bid * (rw * TILES) >= n_out) return;
    const long long tile_row0 = (long long)bid * (rw * TILES) + t * rw;
    const long long row = tile_row0 + r;
    const bool valid = row < n_out && r < rw;
    const int wbeg = (g * NWIN + G - 1) / G, wend = ((g + 1) * NWIN + G - 1) / G;
    const int nw = EVEN ? NWIN / G : wend - wbeg;        // windows of this group
    const int k0 = 3 * wbeg;                             // its first offset
    {   // the tile's 32 x 27 table: each of its G waves brings a share (coalesced 16-byte loads -> LDS)
        const long long tbl_bytes = (long long)n_cap * KVOL * 4;
        const long long left = tbl_bytes - tile_row0 * KVOL * 4;
        const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<int *>(left > 0 ? nbr + tile_row0 * KVOL : nbr), 0, (int)(left <= 0 ? 0 : (left < 32 * KVOL * 4 ? left : 32 * KVOL * 4)), 0x00020000);
#pragma unroll
        for (int i = 0; i < (PER + 63) / 64; ++i) {
            const int q = i * 64 + lane, p16 = g * PER + q;
            if (q < PER && p16 < TBL16) stage[t * TBL16 + p16] = __builtin_amdgcn_raw_buffer_load_b128(trs, p16 * 16, 0, 0);
        }
    }
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(feat), 0, (int)feat_bytes, 0x00020000);
    const u32x4_t *wpv = reinterpret_cast<const u32x4_t *>(packed) + (size_t)k0 * C::BSLOT + (size_t)t * WPW * 64 + lane;
    u32x4_t *wslot = reinterpret_cast<u32x4_t *>(ring) + (size_t)g * 2 * WIN16 + t * WPW * 64 + lane;
    const uint4 *rbase = ring + (size_t)g * 2 * WIN16 + lane;
    const int *tbl = reinterpret_cast<const int *>(stage + t * TBL16) + r * KVOL + k0;
    u32x4_t ww[WPW];
    u32x4_t areg[DIST][4];
    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.0f;
#define SEC_KS_WLOAD(j)                                                                                               \
    {                                                                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < WPW; ++i_) {                                                          \
            if constexpr ((ABL & 2) != 0) ww[i_] = u32x4_t{(unsigned)lane, 0u, 0u, 0u};                                \
            else ww[i_] = wpv[(size_t)(j) * WIN16 + i_ * 64];                                                         \
        }                                                                                                             \
    }
#define SEC_KS_WSTORE(j)                                                                                              \
    {                                                                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < WPW; ++i_) wslot[((j) & 1) * WIN16 + i_ * 64] = ww[i_];                \
    }
#define SEC_KS_GFETCH(lk)                                                                                             \
    {                                                                                                                 \
        const int t_ = valid ? tbl[lk] : -1;                                                                          \
        const unsigned o_ = (t_ >= 0 && (ABL & 1) == 0) ? (unsigned)t_ * 128u + h * 16 : 0x80000000u;                 \
        areg[(lk) % DIST][0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_, 0, 0);                                 \
        areg[(lk) % DIST][1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_ + 32, 0, 0);                            \
        areg[(lk) % DIST][2] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_ + 64, 0, 0);                            \
        areg[(lk) % DIST][3] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o_ + 96, 0, 0);                            \
    }
    SEC_KS_WLOAD(0)
    __syncthreads();                                     // the tile's table is in LDS
#pragma unroll
    for (int lk = 0; lk < DIST; ++lk) SEC_KS_GFETCH(lk)
    SEC_KS_WSTORE(0)
    if (nw > 1) SEC_KS_WLOAD(1)
#pragma unroll
    for (int j = 0; j < WMAX; ++j) {
        __syncthreads();                                 // W of window j is visible; every wave has left the other half of its ring
        if (EVEN || j < nw) {
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const int lk = 3 * j + o;
                uint4 bf[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) bf[i] = rbase[(j & 1) * WIN16 + o * C::BSLOT + i * 64];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const uint4 a = __builtin_bit_cast(uint4, areg[lk % DIST][s]);
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[n] = Mfma<T>::run(bf[s * 2 + n], a, acc[n]);   // D^T
                }
                __builtin_amdgcn_sched_barrier(0);
                if (lk + DIST < 3 * nw) SEC_KS_GFETCH(lk + DIST)
            }
            if (j + 1 < nw) {
                SEC_KS_WSTORE(j + 1)
                if (j + 2 < nw) SEC_KS_WLOAD(j + 2)
            }
        }
    }
#undef SEC_KS_WLOAD
#undef SEC_KS_WSTORE
#undef SEC_KS_GFETCH
    // partial sums of groups 1 .. G-1 -> LDS (over the rings) -> group 0, added in group order
    __syncthreads();                                     // every wave is done with its ring
    float4 *red = reinterpret_cast<float4 *>(ring);
    if (g > 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            red[(((g - 1) * TILES + t) * 8 + i) * 64 + lane] =
                make_float4(acc[i >> 2][(i & 3) * 4], acc[i >> 2][(i & 3) * 4 + 1], acc[i >> 2][(i & 3) * 4 + 2], acc[i >> 2][(i & 3) * 4 + 3]);
    }
    __syncthreads();
    if (g > 0) return;
#pragma unroll
    for (int gg = 1; gg < G; ++gg)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = red[(((gg - 1) * TILES + t) * 8 + i) * 64 + lane];
            acc[i >> 2][(i & 3) * 4] += v.x;
            acc[i >> 2][(i & 3) * 4 + 1] += v.y;
            acc[i >> 2][(i & 3) * 4 + 2] += v.z;
            acc[i >> 2][(i & 3) * 4 + 3] += v.w;
        }
    rows_store<T, 64>(acc, out, row, valid, h, aff, scale != nullptr, shift != nullptr, relu);
}

template <typename T, int TILES, int G, int ABL = 0>
static void launch_rows_ks(const void *feat, long long n_feat, const void *packed, const int *nbr, int n_out, const int *num_out_dev,
                           const float *scale, const float *shift, int relu, void *out, hipStream_t st) {
    using C = RowsCfg<T, 64, 64>;
    set_last_kernel("k_conv_rows_ks<%s, %d, %d>", dtype_name<T>(), TILES, G);
    constexpr size_t lds = (size_t)G * 2 * 3 * C::BSLOT * 16 + (size_t)TILES * (32 * 27 / 4) * 16 + 2 * 64 * sizeof(float);
    auto fn = k_conv_rows_ks<T, TILES, G, ABL>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    int blocks = div_up(n_out, 32 * TILES);
    if (blocks < kBalWgs) blocks = kBalWgs;
    const int xcd = rows_xcd_order();
    if (xcd) blocks = (blocks + 7) / 8 * 8 + 8;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(TILES * G * 64), lds, st, (const T *)feat, n_feat * 64 * (long long)sizeof(T), (const T *)packed,
                       nbr, n_out, num_out_dev, scale, shift, (relu & 1) | (xcd << 16), (T *)out);
}

