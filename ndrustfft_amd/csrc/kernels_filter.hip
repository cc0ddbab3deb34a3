// kernels_filter.hip -- the fused filter (filter_kernel.h): forward transform, weights and inverse transform of a lane in ONE launch, in three modes on the same
// complex kernel of length F.  Same XCD map, load policy and 16-byte rule as launch_pow2 (kernels_pow2.hip).
//   FILTER_C2C  complex lanes of n = F points under a C2C plan: out = s IFFT(w (.) FFT(in)).  Pitches in complex elements.
//   FILTER_R2C  REAL lanes of n = 2 F points under an R2C plan, read as F complex points: the mirror exchange and the pair mix between the two pass sets.  The caller
//               passes pitches in COMPLEX elements (half the real pitches) and bases that are whole complex elements.  Every instance measured 53-67 % below the
//               composed route.
//   FILTER_DCT  REAL lanes of n = 2 F points under a DCT plan: DCT-II, n real weights, DCT-III, between a staged load through Makhoul's permutation and a staged store
//               through its inverse.  Pitches in REALS; any base and any pitch: the accesses are sizeof(T) wide unless both sides are 16-byte aligned, then 16 bytes.
// FILTER_C2C also has a COLUMN form (launch_filter_col, at the end): lanes of n = 128 .. 2048 points along a strided axis whose neighbouring lanes are adjacent in both
// arrays (FilterArgs::inner, outer_*, elem_*), a workgroup per tile of adjacent lanes staged through LDS, the same pass sets and tables.  compose.hip takes it where the
// fastest batch dim has unit stride in both views, there are at most two batch dims and at least 8 adjacent lanes.  The column forms of the other two modes are not written.
#include "pow2_config.h"
#include "filter_kernel.h"

namespace ndfft {

// THE list of shipped instances, by the complex length F (tests/filter_real_suite.py: FUSED_R_N and tests/filter_dct_suite.py: FUSED_D_N mirror it as n = 2 F).  The two
// longest row lengths (PSPLIT forms, 122-126 VGPRs for one pass set) stay on the composed route of compose.hip.
#define NDFFT_FILTER_LENGTHS(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)
static int filter_F(int mode, int n) { return mode == FILTER_C2C ? n : n % 2 == 0 ? n / 2 : 0; }
bool filter_supported(int mode, int dtype, int n) {
    if (mode < FILTER_C2C || mode > FILTER_DCT) return false;
    switch (filter_F(mode, n)) {
#define NDFFT_CASE(N_) case N_: return pow2_supported(dtype, N_);
        NDFFT_FILTER_LENGTHS(NDFFT_CASE)
#undef NDFFT_CASE
        default: return false;
    }
}
// per-pass twiddles of the reversed radix list; empty when the list is a palindrome (the plan's own table serves both pass sets)
void filter_pow2_build_twiddles(int dtype, int n, HostTable &out) {
    switch (n) {
#define NDFFT_CASE(N_, TPL_, ...)                                                                                                         \
    case N_:                                                                                                                              \
        if (dtype == NDFFT_F32) { if (!radix_palindromic<Pow2Cfg<float, N_>::RL>()) build_tw<Reversed<Pow2Cfg<float, N_>::RL>::type>(out); } \
        else if (!radix_palindromic<Pow2Cfg<double, N_>::RL>()) build_tw<Reversed<Pow2Cfg<double, N_>::RL>::type>(out);                    \
        break;
        NDFFT_POW2_CONFIGS_F64(NDFFT_CASE)
#undef NDFFT_CASE
        default: break;
    }
}
// the real modes: per-pass twiddles of the length-F list and of its reverse (empty: a palindrome), F = n / 2
void filter_r2c_build_twiddles(int dtype, int n, HostTable &fwd, HostTable &rev) {
    pow2_build_twiddles(dtype, n / 2, fwd);
    filter_pow2_build_twiddles(dtype, n / 2, rev);
}

template <typename T, int N, int NT, int VEC, int MODE> static int launch_filter_inst(const FilterArgs &f0, hipStream_t s) {
    constexpr int TPL = Pow2Cfg<T, N>::TPL, LPB = lpb_for(TPL);
    using K = FilterKernel<T, N, TPL, LPB, Pow2Half<T, N>::value, typename Pow2Cfg<T, N>::RL, N >= 4096 ? 16 : 0, NT, VEC, MODE>;
    NDFFT_ENSURE_LDS_ATTR((k_filter_pow2<K>));
    const int64_t nblk = (f0.a.nlanes + LPB - 1) / LPB;
    if (nblk <= 0) return NDFFT_OK;
    if (nblk > 0x7fffffffLL) return fail(NDFFT_ERR_UNSUPPORTED, "too many lanes for one launch");
    FilterArgs f = f0;
    f.a.xcd_chunk = xcd_chunk_for((size_t)LPB * N * sizeof(cpx<T>), nblk);
    hipLaunchKernelGGL(k_filter_pow2<K>, dim3((unsigned)nblk), dim3(K::THREADS), K::LDS_BYTES, s, f);
    NDFFT_HIP(hipGetLastError());
    return NDFFT_OK;
}
template <typename T, int N, int VEC, int MODE> static int launch_filter_one(const FilterArgs &f, hipStream_t s) {
    const bool nt_in = f.a.stream_in >= 0 ? f.a.stream_in != 0 : stream_loads_for((size_t)f.a.nlanes * N * sizeof(cpx<T>));
    return nt_in ? launch_filter_inst<T, N, 3, VEC, MODE>(f, s) : launch_filter_inst<T, N, 1, VEC, MODE>(f, s);
}
// VEC: elements per global access -- 1, or what fills 16 bytes where the host found both sides aligned (vec_ok): two complex f32 elements where the radix list
// allows it (f32_can_vec2; complex f64 elements are 16 bytes already), 16 / sizeof(T) reals in the DCT mode
template <int N, int MODE> static int launch_filter_n(int dtype, bool vec_ok, const FilterArgs &f, hipStream_t s) {
    constexpr bool DCT = MODE == FILTER_DCT;
    if (dtype == NDFFT_F64) {
        if constexpr (DCT) { if (vec_ok) return launch_filter_one<double, N, 2, MODE>(f, s); }
        return launch_filter_one<double, N, 1, MODE>(f, s);
    }
    if constexpr (DCT || f32_can_vec2<N>()) { if (vec_ok) return launch_filter_one<float, N, DCT ? 4 : 2, MODE>(f, s); }
    return launch_filter_one<float, N, 1, MODE>(f, s);
}
int launch_filter(int mode, int dtype, int n, const FilterArgs &f, hipStream_t s) {
    static const char *const unsupported[] = {"filter kernel: unsupported n", "real filter kernel: unsupported n", "dct filter kernel: unsupported n"};
    if (mode < FILTER_C2C || mode > FILTER_DCT) return fail(NDFFT_ERR_UNSUPPORTED, "filter kernel: unknown mode");
    if (!filter_supported(mode, dtype, n)) return fail(NDFFT_ERR_UNSUPPORTED, unsupported[mode]);
    // 16-byte accesses need 16-byte aligned bases and pitches of whole 16-byte groups: even pitches of complex elements, 16 / sizeof(T) reals in the DCT mode
    const Pow2Args &a = f.a;
    const int64_t per16 = mode != FILTER_DCT ? 2 : dtype == NDFFT_F64 ? 2 : 4;
    const bool vec_ok = a.pitch_in % per16 == 0 && a.pitch_out % per16 == 0 && ((uintptr_t)a.in % 16) == 0 && ((uintptr_t)a.out % 16) == 0;
    switch (filter_F(mode, n)) {
#define NDFFT_CASE(N_)                                                                      \
    case N_:                                                                                \
        return mode == FILTER_DCT   ? launch_filter_n<N_, FILTER_DCT>(dtype, vec_ok, f, s)  \
               : mode == FILTER_R2C ? launch_filter_n<N_, FILTER_R2C>(dtype, vec_ok, f, s)  \
                                    : launch_filter_n<N_, FILTER_C2C>(dtype, vec_ok, f, s);
        NDFFT_FILTER_LENGTHS(NDFFT_CASE)
#undef NDFFT_CASE
        default: return fail(NDFFT_ERR_UNSUPPORTED, unsupported[mode]);
    }
}

// ---- FILTER_C2C along a strided axis: column tiles (filter_kernel.h: FilterColKernel) ------------------------------------------------------------------------------
// THE list of shipped column instances per dtype: X(length, lanes per tile) (tests/filter_col_suite.py: FUSED_COL_N mirrors the lengths).  The widths start from
// ColGeom<T, N, 0> (kernels_pow2_real.hip) and were settled on 2^24 points along axis 0, HBM-sourced (tools/bench_filter.py --axis 0; profiles/r15/bench_filter_col_ab_*.jsonl;
// us per call, this width against twice / half as many lanes where that fits 1024 threads and 160 KiB):
//   f64  128: 32 lanes 130.6 (64: 145.1, 16: 129.5)   256: 16 lanes 124.6 (32: 147.7, 8: 130.3)   512: 8 lanes 147.5 (16: 163.8, 4: 191.2)
//        1024: 8 lanes 183.1 (4: 215.5; 16 do not fit)   2048: 4 lanes 266.5 (nothing else fits)
//   f32  128: 32 lanes 68.5 (64: 74.7, 16: 70.0)   256: 16 lanes 71.4 (32: 74.6)   512: 16 lanes 74.6 (32: 100.5, 8: 100.0)   1024: 16 lanes 115.2 (8: 118.5)
//        2048: 8 lanes 134.2 (4: 337.3)
// So: a tile of about 70 KiB -- two workgroups per CU, one loading while the other computes -- wherever its rows are still 128 bytes; the long lengths take what fits.
// Every one of these measured 50-65 % below the composed route.  f32 4096 (4 lanes = 32-byte rows, all that fits) measured 255.3 us against 250.2
// composed and is not shipped; f64 4096 has no tile of 4 lanes.  NDFFT_FILTER_COL_WIDE = 1 / -1 (A/B builds) doubles / halves every tile that allows it;
// NDFFT_FILTER_COL_HALF = 1 runs the passes' exchanges component-wise (never faster: f64 2048 292.8 against 266.5, f32 2048 150.6 against 134.2, the rest within 0-9 %).
#define NDFFT_FILTER_COL_LENGTHS_F64(X) X(128, 32) X(256, 16) X(512, 8) X(1024, 8) X(2048, 4)
#define NDFFT_FILTER_COL_LENGTHS_F32(X) X(128, 32) X(256, 16) X(512, 16) X(1024, 16) X(2048, 8)
#ifndef NDFFT_FILTER_COL_WIDE
#define NDFFT_FILTER_COL_WIDE 0
#endif
#ifndef NDFFT_FILTER_COL_HALF
#define NDFFT_FILTER_COL_HALF 0
#endif
template <typename T, int N> struct FilterColCfg { static constexpr int LPB = 0; };
template <typename T, int N, int LPB0> struct FilterColWidth {
    static constexpr int TPL = Pow2Cfg<T, N>::TPL;
    static constexpr size_t LANE_BYTES = (size_t)((N + (N >> 4) + 2) | 1) * 2 * sizeof(T);
    static constexpr bool DOUBLE = NDFFT_FILTER_COL_WIDE > 0 && 2 * LPB0 * TPL <= 1024 && 2 * LPB0 * LANE_BYTES <= 160 * 1024;
    static constexpr bool HALVE = NDFFT_FILTER_COL_WIDE < 0 && LPB0 >= 8;
    static constexpr int LPB = DOUBLE ? 2 * LPB0 : HALVE ? LPB0 / 2 : LPB0;
    static_assert(LPB * TPL <= 1024 && LPB * LANE_BYTES <= 160 * 1024, "a column tile is one workgroup and fits the LDS");
};
#define NDFFT_DEF(N_, LPB_) template <> struct FilterColCfg<double, N_> { static constexpr int LPB = FilterColWidth<double, N_, LPB_>::LPB; };
NDFFT_FILTER_COL_LENGTHS_F64(NDFFT_DEF)
#undef NDFFT_DEF
#define NDFFT_DEF(N_, LPB_) template <> struct FilterColCfg<float, N_> { static constexpr int LPB = FilterColWidth<float, N_, LPB_>::LPB; };
NDFFT_FILTER_COL_LENGTHS_F32(NDFFT_DEF)
#undef NDFFT_DEF
static int filter_col_lanes(int dtype, int n) {      // lanes per tile, 0: no instance
    switch (n) {
#define NDFFT_CASE(N_) case N_: return dtype == NDFFT_F64 ? FilterColCfg<double, N_>::LPB : FilterColCfg<float, N_>::LPB;
        NDFFT_FILTER_LENGTHS(NDFFT_CASE)
#undef NDFFT_CASE
        default: return 0;
    }
}
bool filter_col_supported(int dtype, int n) { return filter_col_lanes(dtype, n) > 0 && pow2_supported(dtype, n); }

// THE column instance of (T, N, load / store policy) (tests/test_filter_col_resources.py reads the compiler's resource remarks of these)
template <typename T, int N, int NT>
using FilterColInst = FilterColKernel<T, N, Pow2Cfg<T, N>::TPL, FilterColCfg<T, N>::LPB, NDFFT_FILTER_COL_HALF != 0, typename Pow2Cfg<T, N>::RL, N >= 4096 ? 16 : 0, NT>;
template <typename T, int N, int NT> static int launch_filter_col_inst(const FilterArgs &f0, hipStream_t s) {
    constexpr int LPB = FilterColCfg<T, N>::LPB;
    if constexpr (LPB == 0) return fail(NDFFT_ERR_UNSUPPORTED, "column filter kernel: unsupported n");
    else {
        using K = FilterColInst<T, N, NT>;
        NDFFT_ENSURE_LDS_ATTR((k_filter_pow2<K>));
        const int64_t nblk = (f0.a.nlanes + LPB - 1) / LPB;
        if (nblk <= 0) return NDFFT_OK;
        if (nblk > 0x7fffffffLL) return fail(NDFFT_ERR_UNSUPPORTED, "too many lanes for one launch");
        FilterArgs f = f0;
        // consecutive tiles are adjacent pieces of the SAME rows: runs of 4 per XCD, the rule of the column transforms (kernels_pow2_real.hip: launch_k)
        f.a.xcd_chunk = nblk >= 64 ? 4 : 0;
        hipLaunchKernelGGL(k_filter_pow2<K>, dim3((unsigned)nblk), dim3(K::THREADS), K::LDS_BYTES, s, f);
        NDFFT_HIP(hipGetLastError());
        return NDFFT_OK;
    }
}
int launch_filter_col(int dtype, int n, const FilterArgs &f, hipStream_t s) {
    if (!filter_col_supported(dtype, n)) return fail(NDFFT_ERR_UNSUPPORTED, "column filter kernel: unsupported n");
    if (f.inner <= 0 || f.inner > f.a.nlanes) return fail(NDFFT_ERR_INVALID_ARG, "column filter kernel: bad inner extent");
    const size_t bytes = (size_t)f.a.nlanes * n * 2 * (dtype == NDFFT_F64 ? sizeof(double) : sizeof(float));
    const bool nt_in = f.a.stream_in >= 0 ? f.a.stream_in != 0 : stream_loads_for(bytes);
    switch (n) {
#define NDFFT_CASE(N_)                                                                                                                              \
    case N_:                                                                                                                                        \
        if (dtype == NDFFT_F64) return nt_in ? launch_filter_col_inst<double, N_, 3>(f, s) : launch_filter_col_inst<double, N_, 1>(f, s);           \
        return nt_in ? launch_filter_col_inst<float, N_, 3>(f, s) : launch_filter_col_inst<float, N_, 1>(f, s);
        NDFFT_FILTER_LENGTHS(NDFFT_CASE)
#undef NDFFT_CASE
        default: return fail(NDFFT_ERR_UNSUPPORTED, "column filter kernel: unsupported n");
    }
}

}  // namespace ndfft
