// pow2_config.h -- which Pow2Kernel instance runs the contiguous-axis C2C FFT of a power-of-two length (kernels_pow2.hip launches them;
// tests/test_pow2_row_resources.py compiles the same instances through Pow2RowKernel and checks their register class).
#pragma once
#include "pow2_kernel.h"

namespace ndfft {

// N, threads-per-lane, radices.  E = N / TPL must be a multiple of every radix.
// f64 (16-byte elements, one element per global access)
#define NDFFT_POW2_CONFIGS_F64(X) \
    X(64, 8, 8, 8)            \
    X(128, 8, 16, 8)          \
    X(256, 16, 16, 16)        \
    X(512, 64, 8, 8, 8)       \
    X(1024, 64, 16, 8, 8)     \
    X(2048, 128, 16, 16, 8)   \
    X(4096, 512, 8, 8, 8, 8)  \
    X(8192, 512, 8, 8, 8, 16) \
    X(16384, 1024, 16, 16, 16, 4)
// f32 (8-byte elements): first and last radix <= E/2 so that two adjacent elements (16 B) move per
// global access (VEC = 2)
#define NDFFT_POW2_CONFIGS_F32(X) \
    X(64, 8, 8, 8)            \
    X(128, 8, 8, 2, 8)        \
    X(256, 16, 8, 4, 8)       \
    X(512, 32, 8, 8, 8)       \
    X(1024, 64, 8, 16, 8)     \
    X(2048, 128, 8, 4, 8, 8)  \
    X(4096, 256, 8, 8, 8, 8)  \
    X(8192, 512, 8, 16, 8, 8) \
    X(16384, 512, 16, 16, 8, 8)

// threads per workgroup (whole lanes): a documented compile-time knob
#ifndef NDFFT_POW2_ROW_THREADS
#define NDFFT_POW2_ROW_THREADS 256
#endif
static constexpr int lpb_for(int tpl) { return tpl >= NDFFT_POW2_ROW_THREADS ? 1 : NDFFT_POW2_ROW_THREADS / tpl; }

template <typename T, int N> struct Pow2Cfg;
#define NDFFT_DEF_CFG64(N_, TPL_, ...) \
    template <> struct Pow2Cfg<double, N_> { static constexpr int TPL = TPL_; using RL = RadixList<__VA_ARGS__>; };
#define NDFFT_DEF_CFG32(N_, TPL_, ...) \
    template <> struct Pow2Cfg<float, N_> { static constexpr int TPL = TPL_; using RL = RadixList<__VA_ARGS__>; };
NDFFT_POW2_CONFIGS_F64(NDFFT_DEF_CFG64)
NDFFT_POW2_CONFIGS_F32(NDFFT_DEF_CFG32)

// LDS exchange: HALF (real parts, then imaginary parts, through one real-sized buffer) halves the footprint and
// wins for f64 (occupancy).  f32 from n = 2048 up exchanges whole complex elements with 64-bit LDS accesses: half
// the LDS instructions, and the footprint is that of the f64 half exchange anyway (measured after the packed-math
// change, tools/kbench f32_halffull: 2048 83 -> 78 us, 4096 86 -> 80, 8192 93 -> 89, 16384 146 -> 126)
template <typename T, int N> struct Pow2Half { static constexpr bool value = true; };
template <> struct Pow2Half<float, 2048> { static constexpr bool value = false; };
template <> struct Pow2Half<float, 4096> { static constexpr bool value = false; };
template <> struct Pow2Half<float, 8192> { static constexpr bool value = false; };
template <> struct Pow2Half<float, 16384> { static constexpr bool value = false; };

// Position-split exchange (pow2_kernel.h: PSPLIT = 2) for the lengths whose lane fills a CU's LDS: two workgroups per CU instead of one.
// NDFFT_PSPLIT=1 / 2 forces it off / on for n = 8192 and 16384 (A/B runs); default: the measured choice below.
// Measured A-B-A-B on 2^24 points (profiles/r05/r05d_psplit_abab.txt): c64 n = 16384 65.5 -> 56.5 us (0.51 -> 0.59 of 8 TB/s), c64 n = 8192 51.8 -> 48.0 us
// (0.65 -> 0.70); c128 n = 16384 unchanged (126 VGPRs x 1024 threads: registers, not LDS, keep it at one workgroup per CU), c128 n = 8192 -2 %.
template <typename T, int N> struct Pow2PSplit { static constexpr int value = (sizeof(T) == 4 && N >= 8192) ? 2 : 1; };

// FLAGS (pow2_kernel.h) of the row kernel of length n; `fused` = with the four-step twiddle on load.
//   bit 4 from n = 4096: late passes whose twiddle table exceeds 32 KiB load W^k, W^2k, W^4k (, W^8k) and build the other powers
//     (2-4 % on the instruction-bound long kernels; two extra roundings on those twiddles)
//   bits 5 + 6, n = 4096 (f64 and f32), plain: the derived latency form -- every pass's power rows are loaded ahead of the exchange in front of it
//     (f64 62 VGPRs, f32 60, 8 waves per SIMD either way; DESIGN.md 3.1 has the measurements, also of the lengths that stayed as they were).
//     The fused instance stays as it was (f64: 71 -> 95 VGPRs, 7 -> 5 waves per SIMD).
template <typename T> constexpr int pow2_row_flags(int n, bool fused) {
    int f = fused ? 8 : 0;
    if (n >= 4096) f |= 16;
    if (n == 4096 && !fused) f |= 32 | 64;
    return f;
}
// THE row kernel: NT = load / store policy, VEC = elements per global access, PS = PSPLIT
template <typename T, int N, int NT, int VEC = 1, bool FUSED = false, int PS = 1>
using Pow2RowKernel = Pow2Kernel<T, N, Pow2Cfg<T, N>::TPL, lpb_for(Pow2Cfg<T, N>::TPL), Pow2Half<T, N>::value, typename Pow2Cfg<T, N>::RL,
                                 pow2_row_flags<T>(N, FUSED), 1, NT, VEC, PS>;

// f32: 16-byte (two-element) accesses where the configuration allows them (an even number of butterflies per
// thread in the first and last pass) and the lanes are 16-byte aligned; n = 64 runs 8 threads x 8 elements with
// 8-byte accesses (measured 92 us vs 106 us for 4 x 16 with 16-byte accesses on 2^25 points)
template <int N> constexpr bool f32_can_vec2() {
    using RL = typename Pow2Cfg<float, N>::RL;
    constexpr int E = N / Pow2Cfg<float, N>::TPL;
    return (E / RL::at(0)) % 2 == 0 && (E / RL::at(RL::NP - 1)) % 2 == 0;
}

}  // namespace ndfft
