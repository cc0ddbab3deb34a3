// kernels_filter.hip -- the fused filter (filter_kernel.h): forward transform, weights and inverse transform of a lane in ONE launch, in three modes on the same
// complex kernel of length F.  Same XCD map, load policy and 16-byte rule as launch_pow2 (kernels_pow2.hip).
//   FILTER_C2C  complex lanes of n = F points under a C2C plan: out = s IFFT(w (.) FFT(in)).  Pitches in complex elements.
//   FILTER_R2C  REAL lanes of n = 2 F points under an R2C plan, read as F complex points: the mirror exchange and the pair mix between the two pass sets.  The caller
//               passes pitches in COMPLEX elements (half the real pitches) and bases that are whole complex elements.  Every instance measured 53-67 % below the
//               composed route.
//   FILTER_DCT  REAL lanes of n = 2 F points under a DCT plan: DCT-II, n real weights, DCT-III, between a staged load through Makhoul's permutation and a staged store
//               through its inverse.  Pitches in REALS; any base and any pitch: the accesses are sizeof(T) wide unless both sides are 16-byte aligned, then 16 bytes.
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

}  // namespace ndfft
