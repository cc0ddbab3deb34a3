// filter_kernel.h -- ndfft_filter on contiguous power-of-two C2C lanes in ONE kernel: out = s IFFT(w (.) FFT(in)), one read and one write of HBM per point.
//
// Pow2Kernel's last pass leaves output element jof<NP-1>(t, q) + r N / R_last in v[q R_last + r]; its first pass wants input element jof<0>(t, q) + r N / R_0 in
// v[q R_0 + r].  Run the inverse transform with the radix list REVERSED and the two coincide: the forward transform's output registers are the inverse's input
// registers, so the product with w needs no exchange and no memory traffic but w itself (<= 64 KiB, L2-resident; the Rader kernel's pointwise product works the
// same way, rader_kernel.h).  The inverse's last pass then stores in the forward's load pattern.  IFFT(y) = conj(FFT(conj(y))): both pass sets are forward ones.
//
// The struct is two Pow2Kernel instantiations over the same (T, N, TPL, LPB, HALF, FLAGS, NT, VEC) and uses their passes<0> only.  Instantiated and launched
// from kernels_pow2.hip (launch_filter_pow2).
//
// REAL: the same on a REAL lane of n = 2N points under an R2C plan (launch_filter_r2c_pow2): out = s IRFFT(w (.) RFFT(in)), w of N + 1 complex values.  The lane is
// read as N complex points z[m] = x[2m] + i x[2m+1] -- the load and the store are the complex kernel's, each complex element two adjacent reals -- and only the step
// between the two pass sets differs: the half spectrum X[k], X[N-k] of the real lane needs Z[k] AND Z[N-k], which another thread holds, so the lane goes through
// its LDS once more (write Z, barrier, gather the mirror bin; the components one after the other where the exchange buffer holds one), and every thread then
// splits, weights and folds its own bins in registers:
//   A = Z[k], B = conj Z[(N-k) mod N], W = e^{-2 pi i k/n}:   X[k] = (A+B)/2 + W (A-B)/(2i),   X[N-k] = conj((A+B)/2 - W (A-B)/(2i))       (k = 0: X[N] is the Nyquist bin)
//   Yk = w[k] X[k], Ym = w[N-k] X[N-k]  (k = 0: both lose their imaginary parts, as ndifft_r2c drops those of DC and Nyquist),   Z'[k] = (Yk + conj Ym) + i conj(W) (Yk - conj Ym)
// The unnormalised inverse FFT_N of Z' is y[2m] + i y[2m+1] with y = n irfft(w (.) rfft(x)).  Both bins of a pair are computed by both threads that hold one of
// them: twice the arithmetic of the split, no second exchange.
#pragma once
#include "pow2_kernel.h"
#include "realops.h"

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

// REAL pair mix: a scheduling fence after every half butterfly round's bins.  Left alone the compiler issues the three table loads of ALL E bins ahead of the
// arithmetic, and their 6 E values are live beside Z and its mirror (4 E): f64 F = 4096 then takes 156 VGPRs = ONE workgroup per CU, fenced 126 = two (n = 8192:
// 113.2 -> 83.4 us on 2^24 points); the f32 16-byte instances of F >= 1024 164-174 -> 124-131 (5-10 % faster).  Where no occupancy step is crossed the fence only
// serialises the loads: f64 F = 128, 1024, 2048 and f32 F = 256 run 5-9 % faster without it, the rest within 1 %, so it is per instance.
// NDFFT_FILTER_MIX_SPLIT = 0 / 2 builds every instance without / with it (A/B libraries).
#ifndef NDFFT_FILTER_MIX_SPLIT
#define NDFFT_FILTER_MIX_SPLIT -1
#endif
template <typename T, int N> constexpr int filter_mix_split() {
    if (NDFFT_FILTER_MIX_SPLIT >= 0) return NDFFT_FILTER_MIX_SPLIT;
    return (sizeof(T) == 8 ? N >= 4096 : N >= 1024) ? 2 : 0;
}
__device__ __forceinline__ void mix_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

template <typename T, int N, int TPL, int LPB, bool HALF, typename RL, int FLAGS, int NT, int VEC, bool REAL = false> struct FilterKernel {
    using RLR = typename Reversed<RL>::type;
    using KF = Pow2Kernel<T, N, TPL, LPB, HALF, RL, FLAGS, 1, NT, VEC>;
    using KI = Pow2Kernel<T, N, TPL, LPB, HALF, RLR, FLAGS, 1, NT, VEC>;
    static constexpr int E = KF::E, THREADS = KF::THREADS, NP = RL::NP, MIX_SPLIT = filter_mix_split<T, N>();
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
        if constexpr (!REAL) {
            const cpx<T> *w = (const cpx<T> *)f.w;
#pragma unroll
            for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                for (int r = 0; r < RZ; ++r) v[q * RZ + r] = cconj(cmul(v[q * RZ + r], w[KF::template jof<NP - 1>(t, q) + r * NBZ]));
        } else {
            // mirror exchange: b[i] = Z[(N - k) mod N] for the bin k of v[i].  The barrier in front of a write: no thread still reads what the write replaces (the last
            // exchange of the first pass set, the other component's round); dead tail lanes take part in every barrier
            cpx<T> b[E];
            if constexpr (HALF) {
                T *s = (T *)lds;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                        for (int r = 0; r < RZ; ++r) s[phi(KF::template jof<NP - 1>(t, q) + r * NBZ)] = half ? v[q * RZ + r].y : v[q * RZ + r].x;
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                        for (int r = 0; r < RZ; ++r) {
                            const T x = s[phi((N - (KF::template jof<NP - 1>(t, q) + r * NBZ)) & (N - 1))];
                            if (half) b[q * RZ + r].y = x; else b[q * RZ + r].x = x;
                        }
                }
            } else {
                cpx<T> *s = (cpx<T> *)lds;
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) s[phi(KF::template jof<NP - 1>(t, q) + r * NBZ)] = v[q * RZ + r];
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) b[q * RZ + r] = s[phi((N - (KF::template jof<NP - 1>(t, q) + r * NBZ)) & (N - 1))];
            }
            // pair mix (the formulas at the top; r2c_split_pair and herm_fold of realops.h on registers).  w: N + 1 values, default cache policy; wn[k] = W_n^k, k <= N
            const cpx<T> *w = (const cpx<T> *)f.w, *wn = (const cpx<T> *)f.wn;
#pragma unroll
            for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                for (int r = 0; r < RZ; ++r) {
                    const int k = KF::template jof<NP - 1>(t, q) + r * NBZ;
                    const cpx<T> A = v[q * RZ + r], B = cconj(b[q * RZ + r]), W = wn[k];
                    const cpx<T> e = mk<T>((A.x + B.x) * (T)0.5, (A.y + B.y) * (T)0.5);
                    const cpx<T> o = cmul(mk<T>((A.y - B.y) * (T)0.5, -(A.x - B.x) * (T)0.5), W);
                    cpx<T> yk = cmul(w[k], cadd(e, o)), ym = cmul(w[N - k], cconj(csub(e, o)));
                    if (k == 0) { yk.y = (T)0; ym.y = (T)0; }
                    v[q * RZ + r] = herm_fold<T>(yk, cconj(ym), W);      // conj(Z'[k]): the inverse runs forward passes
                    if constexpr (MIX_SPLIT > 0) { if ((r + 1) % (RZ / MIX_SPLIT) == 0) mix_fence(); }
                }
        }
        // (the first exchange of the second pass set starts with a barrier: no thread overwrites LDS another still reads from the first set's last exchange, or gathers from)
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
