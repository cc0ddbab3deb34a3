// kernels_pow2.hip -- the north-star kernel: batched C2C FFT along the contiguous axis,
// power-of-two n, ONE read and ONE write of HBM per point (BASELINE cfg2 / cfg5 / cfg3-B).
//
// Replaces, per lane, FftHandler::fft_lane / ifft_lane (src/lib.rs:313-331) together with the
// strategy-(i) row loop that calls it (src/lib.rs:117-124, par 187-194).
//
// Design (CDNA4):
//  * A lane lives in REGISTERS: TPL threads x E = n/TPL complex elements each.  The first radix
//    pass reads global memory directly in the Stockham input pattern x[j + r n/R] -- consecutive
//    threads, consecutive 16-byte elements, 1 KiB per wave instruction -- and the last pass writes
//    y[j + r n/R] the same way, so there is no staging copy on either side.
//  * Between passes the lane is exchanged through LDS at its natural Stockham index, padded by one
//    element every 16 (phi(p) = p + p/16) so the stride-R writes of early passes and the unit
//    stride reads of the next pass are both bank-conflict free.
//  * HALF exchange: real parts, then imaginary parts, through ONE real-sized buffer.  n=4096 f64
//    needs 34 KiB instead of 68 KiB, i.e. 4 workgroups per CU instead of 2 -- the occupancy that
//    keeps enough HBM requests in flight while other workgroups are in their butterfly phase.
//  * Twiddles come from per-pass tables laid out [r-1][k] so that a wave reads them coalesced;
//    they are built on the host in long double (plan.hip) and stay L2-resident (<= 64 KiB).
//  * Streaming cache policy: non-temporal stores (and loads, for inputs larger than the Infinity
//    Cache) -- see launch_pow2.
//  * No MFMA: ~1.9 flop/byte, the kernel is HBM-bound by design.
#include <algorithm>
#include <cstdlib>

#include "pow2_config.h"

namespace ndfft {

bool pow2_supported(int dtype, int n) {
    (void)dtype;
    switch (n) {
#define NDFFT_CASE(N_, TPL_, ...) case N_: return true;
        NDFFT_POW2_CONFIGS_F64(NDFFT_CASE)
#undef NDFFT_CASE
        default: return false;
    }
}

void pow2_build_twiddles(int dtype, int n, HostTable &out) {
    switch (n) {
#define NDFFT_CASE(N_, TPL_, ...) \
    case N_: if (dtype == NDFFT_F32) build_tw<Pow2Cfg<float, N_>::RL>(out); else build_tw<Pow2Cfg<double, N_>::RL>(out); break;
        NDFFT_POW2_CONFIGS_F64(NDFFT_CASE)
#undef NDFFT_CASE
        default: break;
    }
}

// Lane blocks per XCD chunk of the workgroup -> lane map (device_common.h: xcd_block): every XCD streams contiguous
// runs of ~512 KiB instead of every eighth lane block.  Measured with tools/kbench f64_map on 4096-point c128 lanes
// (profiles/r02c_*): cache-cold 2 GiB arrays 5.56 -> 6.09 TB/s (6.24 with streaming loads), Infinity-Cache-warm
// 4096 x 4096 6.58 -> 6.85 TB/s; runs of 128 KiB .. 8 MiB are within 2 % of each other, one eighth of the array per
// XCD is worse when cold.  NDFFT_XCD_CHUNK_KB overrides the run length (0 = identity map).
int xcd_chunk_for(size_t block_bytes, int64_t nblk) {
    const long kb = NDFFT_DEV_INT("NDFFT_XCD_CHUNK_KB", 512);
    if (kb <= 0 || block_bytes == 0) return 0;
    if (block_bytes >= ((size_t)256 << 10)) return 0;   // one workgroup already streams >= 256 KiB (n = 16384): the map only cost there (0.54 -> 0.50)
    int64_t c = (int64_t)((size_t)kb * 1024 / block_bytes);
    if (c < 1) c = 1;
    if (nblk < 16 * c) return 0;              // fewer than two whole groups: nothing to gain
    return (int)std::min<int64_t>(c, 1 << 20);
}
// Inputs well beyond the 256 MiB Infinity Cache (> 384 MiB) cannot be resident in it: they are loaded with the streaming (nt)
// policy (cache-cold 2 GiB arrays: +3 % alone, +8..12 % together with the XCD map).  Smaller inputs keep the default
// policy: if their producer left them in the Infinity Cache plain loads are up to 15 % faster (4096 x 4096 c128:
// 0.86 vs 0.74 of the roofline), if not they cost 6 % (0.70 vs 0.74) -- the asymmetric bet; a 268 MB input that the bench loop
// re-reads (cfg3-B) still ran 88 us with plain loads vs 99 us streaming, hence the margin above 256 MiB.  NDFFT_STREAM_LOADS=0/1 forces it.
bool stream_loads_for(size_t in_bytes) {
    const int force = sw().stream_loads;             // NDFFT_STREAM_LOADS
    if (force >= 0) return force != 0;
    return in_bytes > ((size_t)384 << 20);
}

// Position-split exchange: pow2_config.h (Pow2PSplit); NDFFT_PSPLIT=1 / 2 forces it off / on for n = 8192 and 16384 (A/B runs)
static int psplit_override() { return (int)NDFFT_DEV_INT("NDFFT_PSPLIT", 0); }

template <typename T, int N, int NT, int VEC, int FL, int PS> static int launch_inst_ps(const Pow2Args &a0, hipStream_t s) {
    constexpr int TPL = Pow2Cfg<T, N>::TPL, LPB = lpb_for(TPL);
    static_assert((FL & ~8) == 0, "callers choose the fused four-step form only; every other flag is pow2_config.h's choice");
    using K = Pow2RowKernel<T, N, NT, VEC, (FL & 8) != 0, PS>;
    NDFFT_ENSURE_LDS_ATTR((k_pow2<K>));
    const int64_t nblk = (a0.nlanes + LPB - 1) / LPB;
    if (nblk <= 0) return NDFFT_OK;
    if (nblk > 0x7fffffffLL) return fail(NDFFT_ERR_UNSUPPORTED, "too many lanes for one launch");
    Pow2Args a = a0;
    a.xcd_chunk = xcd_chunk_for((size_t)LPB * N * sizeof(cpx<T>), nblk);
    // the kept share counts blocks of 64 KiB of a DENSE input (a lane of that size or more is its own block); a pitched one keeps nothing
    constexpr size_t lane_bytes = (size_t)N * sizeof(cpx<T>);
    a.keep_shift = 0;
    for (size_t b = lane_bytes; b < ((size_t)64 << 10); b <<= 1) ++a.keep_shift;
    if ((NT & 4) == 0) a.keep64 = 0;
    // developer knob (A/B only): extra dynamic LDS per workgroup = fewer resident workgroups per CU
    const size_t pad = (size_t)NDFFT_DEV_INT("NDFFT_POW2_LDS_PAD_KB", 0) << 10;
    hipLaunchKernelGGL(k_pow2<K>, dim3((unsigned)nblk), dim3(K::THREADS), std::min(K::LDS_BYTES + pad, (size_t)160 * 1024), s, a);
    NDFFT_HIP(hipGetLastError());
    return NDFFT_OK;
}
template <typename T, int N, int NT, int VEC, int FL = 0> static int launch_inst(const Pow2Args &a, hipStream_t s) {
    if constexpr (N >= 8192) {   // both forms exist for the two longest lengths (shorter ones: within +-2 % either way, profiles/r05/r05k_psplit_1024_4096.txt)
        const int ov = psplit_override();
        const int ps = ov == 1 || ov == 2 ? ov : Pow2PSplit<T, N>::value;
        return ps == 2 ? launch_inst_ps<T, N, NT, VEC, FL, 2>(a, s) : launch_inst_ps<T, N, NT, VEC, FL, 1>(a, s);
    } else {
        return launch_inst_ps<T, N, NT, VEC, FL, 1>(a, s);
    }
}
template <typename T, int N, int NT, int VEC, int FL = 0> static int launch_one(const Pow2Args &a, hipStream_t s) {
    static_assert(NT == 1, "callers name the store policy; the load policy is chosen here");
    const bool nt_in = a.stream_in >= 0 ? a.stream_in != 0 : stream_loads_for((size_t)a.nlanes * N * sizeof(cpx<T>));
    // a kept share (Pow2Args::keep64, dense inputs) runs the instance that carries the per-lane choice; everything else the one it always ran
    if constexpr (FL == 0) {
        if (nt_in && a.keep64 > 0 && a.pitch_in == N) return launch_inst<T, N, 7, VEC, FL>(a, s);
    }
    if (nt_in) return launch_inst<T, N, 3, VEC, FL>(a, s);
    return launch_inst<T, N, 1, VEC, FL>(a, s);
}

// f32: 16-byte (two-element) accesses where the configuration allows them (pow2_config.h: f32_can_vec2) and the lanes are 16-byte aligned
template <int N> static int launch_f32(bool vec_ok, bool fused, const Pow2Args &a, hipStream_t s) {
    if constexpr (f32_can_vec2<N>()) {
        if (vec_ok) return fused ? launch_one<float, N, 1, 2, 8>(a, s) : launch_one<float, N, 1, 2>(a, s);
    }
    return fused ? launch_one<float, N, 1, 1, 8>(a, s) : launch_one<float, N, 1, 1>(a, s);
}

// Cache policy (measured, tools/kbench.hip f64_4096 sweep over 4096..16384 lanes): the output is
// always stored non-temporally (4096x4096 c128: 84 us vs 105 us with plain stores); the input is
// loaded with the default policy at every size -- non-temporal loads cost 9 % while the input still
// fits the 256 MiB Infinity Cache and are within +-2 % of plain loads beyond it.
// The fused four-step twiddle (Pow2Args::twlo) is its own instantiation (FLAGS bit 3): as a
// run-time branch it cost the plain kernel 23-70 VGPRs (n=8192 f64: 122 -> 194, one block per CU).
int launch_pow2(int dtype, int n, const Pow2Args &a, hipStream_t s) {
    // 16-byte accesses for f32 need even pitches and 16-byte aligned bases
    const bool vec_ok = a.pitch_in % 2 == 0 && a.pitch_out % 2 == 0 && ((uintptr_t)a.in % 16) == 0 && ((uintptr_t)a.out % 16) == 0;
    const bool fused = a.twlo != nullptr;
    switch (n) {
#define NDFFT_CASE(N_, TPL_, ...)                                                               \
    case N_:                                                                                    \
        if (dtype == NDFFT_F64) return fused ? launch_one<double, N_, 1, 1, 8>(a, s) : launch_one<double, N_, 1, 1>(a, s); \
        return launch_f32<N_>(vec_ok, fused, a, s);
        NDFFT_POW2_CONFIGS_F64(NDFFT_CASE)
#undef NDFFT_CASE
        default: return fail(NDFFT_ERR_UNSUPPORTED, "pow2 kernel: unsupported n");
    }
}

}  // namespace ndfft

// kernels_filter.hip is a unit of its own (-DNDFFT_FILTER_UNIT, set by every build list that names it).  A list of objects written before it existed expects
// the filter launchers here: such a build gets them through this unit.
#ifndef NDFFT_FILTER_UNIT
#include "kernels_filter.hip"
#endif
