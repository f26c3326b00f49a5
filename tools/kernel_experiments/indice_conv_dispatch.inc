// Dispatch of the A/B kernels of -DSEC_CONV_EXPERIMENTS builds (and of the timing-only forms of -DSEC_CONV_ABLATIONS): everything such a
// build adds to the plan and launch logic of indice_conv.hip, behind ONE plan hook (experiment_plan, called by conv_fwd_decide after the
// shipped decision) and ONE launch hook (experiment_launch, called by launch_mfma before the shipped kernels).  Included by
// indice_conv.hip inside namespace sec, after the shipped plan ids, variant numbers, row-split forms and launch_rows_buf.
//
// Variant numbers of sec_indice_conv_set_variant that only these builds honour (16-bit features with a packed weight; the row-split
// forms also need out_dtype = dtype and a feature matrix):
//    2, 3      weights / weights and rows staged in LDS (k_conv_mfma_lds, k_conv_mfma_lds2; 27 offsets)                    plan 99
//    4, 5      split-K with two / one row tiles per workgroup (k_conv_mfma_skm)                                            plan 99
//    6, 7      workgroup-wide weight slices in LDS (k_conv_wlds; 7: k_conv_wlds_fl for Cin 32 / 64)                        plan 99
//    9         the first row-split form, LDS-DMA operands (k_conv_rows; Cin, Cout in {32, 64}, 27 offsets)                 plan 6
//    10-12     its compacted / touch-ordered forms (Cin 64)                                                                plans 7-9
//    13-15     register-direct gathers (k_conv_rows_reg, 64 -> 64)                                                         plan 10
//    16-21, 23, 27, 28   k_conv_rows_buf, 64 -> 64: staging / pipelining off, prefetch distance, 4 or 8 waves, skew        plan 11
//    24-26, 44, 45, 60-67   (ablation builds) k_conv_rows_buf, 64 -> 64, timing-only forms; other builds: the forced shipped form
//    36-40     k_conv_rows_buf, Cin <= 32: prefetch distance 6 / 8 / 12, the all-weights form at distance 4 / 6                plan 11
//    41        two row tiles per wave (k_conv_rows_m2, 64 -> 64; 42, 43: its ablations)                                    plan 13
//    46        input planes staged in LDS windows (k_conv_rows_lds, 64 -> 64)                                              plan 14
//    50        the offsets of a row tile split over three wave groups (k_conv_rows_ks, 64 -> 64; 71-73: its ablations)     plan 15
//    91-96     (ablation builds) timing-only forms of k_conv_rows, 64 -> 64; the plan query keeps answering split-K
// SEC_CONV_KS=1 makes k_conv_rows_ks the automatic choice of the mid-size 64 -> 64 layers (A/B: measured slower than the four-wave form of
// k_conv_rows_buf); the two-tiles-per-wave kernel as the automatic choice of the large ones was measured slower too (kM2Auto).
static bool ks_auto() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("SEC_CONV_KS"); v = e ? atoi(e) != 0 : 0; }
    return v != 0;
}
constexpr bool kM2Auto = false;

// `p` holds the shipped decision for (v, xshare); `fits`: the feature matrix is addressable by a raw buffer resource
static void experiment_plan(int cin, int cout, int kvol, int rows, bool same_dtype, bool has_feat, bool fits, int v, int xshare, ConvPlan *p) {
    if (v >= 2 && v <= 7) { p->id = PLAN_EXPERIMENT; return; }
    if (!same_dtype || !has_feat) return;
    const bool c64 = cin == 64 && cout == 64 && kvol == 27;
    if (buf_shape(cin, cout, kvol)) {
        int id = 0;
        if (c64 && v == 46) id = PLAN_ROWS_LDS;
        else if (c64 && (v == 41 || v == 42 || v == 43 || (v == kVarAuto && kM2Auto && rows >= kRowsMin))) id = PLAN_ROWS_M2;
        else if (c64 && (v == 50 || (v >= 71 && v <= 73) || (v == kVarAuto && rows >= kRowsMinSmall && rows < kRowsMin && ks_auto()))) id = PLAN_ROWS_KS;
        // A/B forms of k_conv_rows_buf; a number without a form in this build (24-26 ... without the ablations) = the forced shipped form
        else if ((c64 && ((v >= 16 && v <= 28) || v == 44 || v == 45 || (v >= 60 && v <= 67))) || (v >= 36 && v <= 40)) id = PLAN_ROWS_BUF;
        if (id) {
            if (fits) *p = {id, id == PLAN_ROWS_BUF ? rows_form(cin, cout, kvol, false, xshare) : kRowsNone};
            return;
        }
    }
    if (p->id == PLAN_ROWS_BUF || kvol != 27 || !(cin == 64 || cin == 32) || !(cout == 64 || cout == 32)) return;
    int id = 0;
    if (cin == 64) {
        if (v == 10) id = PLAN_ROWS_COMPACT;
        else if (v == 11) id = PLAN_ROWS_TOUCH;
        else if (v == 12) id = PLAN_ROWS_COMPACT_TOUCH;
        else if (v >= 13 && v <= 15 && cout == 64) id = PLAN_ROWS_REG;
    }
    if (!id && v == 9) id = PLAN_ROWS;
    if (id) *p = {id, kRowsNone};
}

template <typename T>
static void launch_rows_lds(const void *feat, long long n_feat, const void *packed, const int *nbr, int n_out, const int *num_out_dev,
                            const float *scale, const float *shift, int relu, void *out, hipStream_t st) {
    set_last_kernel("k_conv_rows_lds<%s>", dtype_name<T>());
    hipLaunchKernelGGL((k_conv_rows_lds<T>), dim3(div_up(n_out, 256)), dim3(256), 0, st, (const T *)feat,
                       n_feat * 64 * (long long)sizeof(T), (const T *)packed, nbr, n_out, num_out_dev, scale, shift, relu, (T *)out);
}

// true: launched.  false: the shipped kernels of launch_mfma take the plan (an experiment plan without a kernel for this launch, such as
// variant 2 on a three-offset layer, ends in split-K there)
template <typename T, typename OT, int CIN, int COUT>
static bool experiment_launch(const ConvPlan &p, const void *feat, long long n_feat, const void *packed, const int *nbr, int n_out,
                              const int *num_out_dev, int kvol, const float *scale, const float *shift, int relu, void *out, hipStream_t st) {
    const int v = conv_variant();
    if constexpr (std::is_same<T, OT>::value && CIN == 64 && COUT == 64) {
        if (p.id == PLAN_ROWS_M2) { launch_rows_m2<T>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st); return true; }
        if (p.id == PLAN_ROWS_LDS) { launch_rows_lds<T>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st); return true; }
        if (p.id == PLAN_ROWS_KS) {
#ifdef SEC_CONV_ABLATIONS
            if (v == 71) { launch_rows_ks<T, 4, 3, 2>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st); return true; }
            if (v == 72) { launch_rows_ks<T, 4, 3, 1>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st); return true; }
            if (v == 73) { launch_rows_ks<T, 4, 3, 3>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st); return true; }
#endif
            launch_rows_ks<T, 4, 3>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
            return true;
        }
    }
    // A/B forms of the buffer-load kernel: prefetch distance, 4- or 8-wave workgroups, staging / pipelining off, skew
    if constexpr (std::is_same<T, OT>::value && buf_shape(CIN, COUT, 27)) {
        if (p.id == PLAN_ROWS_BUF && kvol == 27) {
#define SEC_BUF(D, W, M, FLG) launch_rows_buf<T, CIN, COUT, D, W, M, FLG, 27>(feat, n_feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st)
            constexpr int kFlPlain = kFlStage + kFlPipe;
            if constexpr (CIN <= 32) {     // narrow layers: a gather is 1-2 registers per offset, deeper prefetch is nearly free
                switch (v) {
                case 36: SEC_BUF(6, 8, 2, kFlPlain); return true;
                case 37: SEC_BUF(8, 8, 2, kFlPlain); return true;
                case 38: SEC_BUF(12, 8, 2, kFlPlain); return true;
                case 39: if constexpr (COUT <= 32) { SEC_BUF(4, 8, 2, kFlPlain + kFlAllW); return true; } break;
                case 40: if constexpr (COUT <= 32) { SEC_BUF(6, 8, 2, kFlPlain + kFlAllW); return true; } break;
                default: break;
                }
            }
            if constexpr (CIN == 64 && COUT == 64) {
                switch (v) {
                case 16: SEC_BUF(4, 4, 2, 0); return true;
                case 17: SEC_BUF(4, 4, 2, kFlStage); return true;
                case 18: SEC_BUF(4, 4, 2, kFlPipe); return true;
                case 19: SEC_BUF(4, 4, 2, kFlPlain); return true;
                case 20: SEC_BUF(5, 4, 2, kFlPlain); return true;
                case 21: SEC_BUF(5, 8, 2, kFlPlain); return true;
                case 23: SEC_BUF(6, 4, 2, kFlPlain); return true;
                case 27: SEC_BUF(5, 8, 2, kFlPlain + kFlSkew); return true;
                case 28: SEC_BUF(6, 8, 2, kFlPlain + kFlSkew); return true;
#ifdef SEC_CONV_ABLATIONS
                case 24: SEC_BUF(4, 8, 2, kFlPlain + kFlAblNoGather); return true;
                case 25: SEC_BUF(4, 8, 2, kFlPlain + kFlAblFewLines); return true;
                case 26: SEC_BUF(4, 8, 2, kFlPlain + kFlAblOneLine); return true;
                // 60-65 (round 6): the shipped four-wave (23 k rows) and eight-wave (56 k rows) forms without the W stream, without gathers that
                // touch memory, without both; 66 / 67: the plain four- / eight-wave form, any row count
                case 60: SEC_BUF(3, 4, 2, kFl64 + kFlAblNoWeights); return true;
                case 61: SEC_BUF(3, 4, 2, kFl64 + kFlAblNoGather); return true;
                case 62: SEC_BUF(3, 4, 2, kFl64 + kFlAblNoWeights + kFlAblNoGather); return true;
                case 63: SEC_BUF(3, 8, 3, kFl64 + kFlAblNoWeights); return true;
                case 64: SEC_BUF(3, 8, 3, kFl64 + kFlAblNoGather); return true;
                case 65: SEC_BUF(3, 8, 3, kFl64 + kFlAblNoWeights + kFlAblNoGather); return true;
                case 66: SEC_BUF(3, 4, 2, kFl64); return true;
                case 67: SEC_BUF(3, 8, 3, kFl64); return true;
                case 44: SEC_BUF(3, 8, 3, kFlStage + kFlLazy + kFlWin3 + kFlAblNoGather); return true;
                case 45: SEC_BUF(3, 8, 3, kFlStage + kFlLazy + kFlWin3 + kFlAblOneLine); return true;
#endif
                default: break;
                }
            }
#undef SEC_BUF
        }
    }
    if constexpr (std::is_same<T, OT>::value && (CIN == 64 || CIN == 32) && (COUT == 64 || COUT == 32)) {
        if constexpr (CIN == 64) {
            if (p.id == PLAN_ROWS_COMPACT) { launch_rows<T, CIN, COUT, 32>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); return true; }
            if (p.id == PLAN_ROWS_TOUCH) { launch_rows<T, CIN, COUT, 64>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); return true; }
            if (p.id == PLAN_ROWS_COMPACT_TOUCH) { launch_rows<T, CIN, COUT, 96>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); return true; }
            if constexpr (COUT == 64) {
                if (p.id == PLAN_ROWS_REG) {
                    if (v == 13) launch_rows_reg<T, CIN, COUT, 4, 2>(feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
                    else if (v == 14) launch_rows_reg<T, CIN, COUT, 2, 3>(feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
                    else launch_rows_reg<T, CIN, COUT, 5, 2>(feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
                    return true;
                }
            }
        }
        if (p.id == PLAN_ROWS) { launch_rows<T, CIN, COUT, 0>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); return true; }
#ifdef SEC_CONV_ABLATIONS
        if (v >= 91 && v <= 96 && kvol == 27 && feat && CIN == 64 && COUT == 64) {
            switch (v) {
            case 91: launch_rows<T, CIN, COUT, 1>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            case 92: launch_rows<T, CIN, COUT, 2>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            case 93: launch_rows<T, CIN, COUT, 4>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            case 94: launch_rows<T, CIN, COUT, 8>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            case 95: launch_rows<T, CIN, COUT, 16>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            default: launch_rows<T, CIN, COUT, 3>(feat, packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, out, st); break;
            }
            return true;
        }
#endif
    }
    // measured dead ends (DESIGN.md section 4)
    if (v == 2 && kvol == 27) {
        hipLaunchKernelGGL((k_conv_mfma_lds<T, OT, CIN, COUT, 27>), dim3(div_up(n_out, 128)), dim3(kBlock), 0, st,
                           (const T *)feat, (const T *)packed, nbr, n_out, num_out_dev, scale, shift, relu, (OT *)out);
        return true;
    }
    if (v == 7 && kvol == 27 && CIN <= 64 && CIN >= 32) {
        launch_wlds_fl<T, OT, CIN, COUT>(feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
        return true;
    }
    if ((v == 6 || v == 7) && kvol == 27 && CIN <= 64) {
        launch_wlds<T, OT, CIN, COUT>(feat, packed, nbr, n_out, num_out_dev, scale, shift, relu, out, st);
        return true;
    }
    if (v == 3 && kvol == 27) {
        hipLaunchKernelGGL((k_conv_mfma_lds2<T, OT, CIN, COUT, 27>), dim3(div_up(n_out, 128)), dim3(kBlock), 0, st,
                           (const T *)feat, (const T *)packed, nbr, n_out, num_out_dev, scale, shift, relu, (OT *)out);
        return true;
    }
    if (v == 4 || v == 5) {
        if (v == 4)
            hipLaunchKernelGGL((k_conv_mfma_skm<T, OT, CIN, COUT, 2>), dim3(div_up(n_out, 64)), dim3(kBlock), 0, st,
                               (const T *)feat, (const T *)packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, (OT *)out);
        else
            hipLaunchKernelGGL((k_conv_mfma_skm<T, OT, CIN, COUT, 1>), dim3(div_up(n_out, 32)), dim3(kBlock), 0, st,
                               (const T *)feat, (const T *)packed, nbr, n_out, num_out_dev, kvol, scale, shift, relu, (OT *)out);
        return true;
    }
    return false;
}
