// filter_kernel.h -- ndfft_filter on contiguous power-of-two C2C lanes in ONE kernel: out = s IFFT(w (.) FFT(in)), one read and one write of HBM per point.
//
// Pow2Kernel's last pass leaves output element jof<NP-1>(t, q) + r N / R_last in v[q R_last + r]; its first pass wants input element jof<0>(t, q) + r N / R_0 in
// v[q R_0 + r].  Run the inverse transform with the radix list REVERSED and the two coincide: the forward transform's output registers are the inverse's input
// registers, so the product with w needs no exchange and no memory traffic but w itself (<= 64 KiB, L2-resident; the Rader kernel's pointwise product works the
// same way, rader_kernel.h).  The inverse's last pass then stores in the forward's load pattern.  IFFT(y) = conj(FFT(conj(y))): both pass sets are forward ones.
//
// The struct is two Pow2Kernel instantiations over the same (T, N, TPL, LPB, HALF, FLAGS, NT, VEC) and uses their passes<0> only.  Instantiated and launched
// from kernels_pow2.hip (launch_filter_pow2).
#pragma once
#include "pow2_kernel.h"

namespace ndfft {

// RadixList back to front
template <typename Out, int... Rs> struct RadixRev;
template <int... Os> struct RadixRev<RadixList<Os...>> { using type = RadixList<Os...>; };
template <int... Os, int R, int... Rs> struct RadixRev<RadixList<Os...>, R, Rs...> { using type = typename RadixRev<RadixList<R, Os...>, Rs...>::type; };
template <typename RL> struct Reversed;
template <int... Rs> struct Reversed<RadixList<Rs...>> { using type = typename RadixRev<RadixList<>, Rs...>::type; };
template <typename RL> constexpr bool radix_palindromic() {
    for (int i = 0; i < RL::NP; ++i) if (RL::at(i) != RL::at(RL::NP - 1 - i)) return false;
    return true;
}

template <typename T, int N, int TPL, int LPB, bool HALF, typename RL, int FLAGS, int NT, int VEC> struct FilterKernel {
    using RLR = typename Reversed<RL>::type;
    using KF = Pow2Kernel<T, N, TPL, LPB, HALF, RL, FLAGS, 1, NT, VEC>;
    using KI = Pow2Kernel<T, N, TPL, LPB, HALF, RLR, FLAGS, 1, NT, VEC>;
    static constexpr int E = KF::E, THREADS = KF::THREADS, NP = RL::NP;
    static constexpr size_t LDS_BYTES = KF::LDS_BYTES;
    static constexpr int R0 = RL::at(0), NB0 = N / R0, NBF0 = KF::slots(0);                  // first pass of the forward list = last pass of the reversed one
    static constexpr int RZ = RL::at(NP - 1), NBZ = N / RZ, NBFZ = KF::slots(NP - 1);        // last pass of the forward list = first pass of the reversed one
    static_assert(KI::E == E && E * TPL == N, "both lists run whole butterfly rounds on the same registers");
    static_assert(KF::full(0) && KF::full(NP - 1), "whole rounds in the first and last pass");
    static_assert(VEC == 1 || (NBF0 % 2 == 0 && NBFZ % 2 == 0), "VEC = 2 needs an even number of butterfly rounds in the first and last pass");
    static_assert((FLAGS & ~16) == 0, "product flags other than the derived twiddle powers have no meaning here");

    static __device__ __forceinline__ void run(const FilterArgs &f) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        const Pow2Args &a = f.a;
        const int t = threadIdx.x % TPL, ll = threadIdx.x / TPL;
        const int64_t lane = (int64_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_chunk) * LPB + ll;
        const bool live = lane < a.nlanes;      // a dead tail lane reads lane 0 and stays in both pass sets (their exchanges have workgroup barriers)
        const cpx<T> *in = (const cpx<T> *)a.in + (live ? lane : 0) * a.pitch_in;
        cpx<T> *out = (cpx<T> *)a.out + (live ? lane : 0) * a.pitch_out;
        char *lds = smem + (size_t)ll * KF::LANE_LDS * (HALF ? sizeof(T) : 2 * sizeof(T));
        cpx<T> v[E];
        if constexpr (VEC == 2) {
#pragma unroll
            for (int q = 0; q < NBF0; q += 2)
#pragma unroll
                for (int r = 0; r < R0; ++r) {
                    const vec4f x = gload4<(NT & 2) != 0>((const float *)(in + KF::template jof<0>(t, q) + r * NB0));
                    v[q * R0 + r] = mk<T>(x.x, x.y); v[(q + 1) * R0 + r] = mk<T>(x.z, x.w);
                }
        } else {
#pragma unroll
            for (int q = 0; q < NBF0; ++q)
#pragma unroll
                for (int r = 0; r < R0; ++r) v[q * R0 + r] = gload<T, (NT & 2) != 0>(in + t + q * TPL + r * NB0);
        }
        KF::template passes<0>(v, (const cpx<T> *)a.twp, lds, t);
        // v[q RZ + r] is bin jof<NP-1>(t, q) + r NBZ: times its weight (default cache policy: every lane reads the same vector), conjugated for the inverse
        {
            const cpx<T> *w = (const cpx<T> *)f.w;
#pragma unroll
            for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                for (int r = 0; r < RZ; ++r) v[q * RZ + r] = cconj(cmul(v[q * RZ + r], w[KF::template jof<NP - 1>(t, q) + r * NBZ]));
        }
        // (the first exchange of the second pass set starts with a barrier: no thread overwrites LDS another still reads from the first set's last exchange)
        KI::template passes<0>(v, (const cpx<T> *)f.twp_rev, lds, t);
        if (!live) return;
        const T sc = (T)a.scale;
#pragma unroll
        for (int i = 0; i < E; ++i) { v[i].x *= sc; v[i].y *= -sc; }
        if constexpr (VEC == 2) {
#pragma unroll
            for (int q = 0; q < NBF0; q += 2)
#pragma unroll
                for (int r = 0; r < R0; ++r) {
                    vec4f x; x.x = v[q * R0 + r].x; x.y = v[q * R0 + r].y; x.z = v[(q + 1) * R0 + r].x; x.w = v[(q + 1) * R0 + r].y;
                    gstore4<(NT & 1) != 0>((float *)(out + KI::template jof<NP - 1>(t, q) + r * NB0), x);
                }
        } else {
#pragma unroll
            for (int q = 0; q < NBF0; ++q)
#pragma unroll
                for (int r = 0; r < R0; ++r) gstore<T, (NT & 1) != 0>(out + t + q * TPL + r * NB0, v[q * R0 + r]);
        }
    }
};

template <typename K> __global__ __launch_bounds__(K::THREADS, 1) void k_filter_pow2(const FilterArgs f) { K::run(f); }

}  // namespace ndfft
