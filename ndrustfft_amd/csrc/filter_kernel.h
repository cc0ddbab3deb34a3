// filter_kernel.h -- ndfft_filter on contiguous power-of-two C2C lanes in ONE kernel: out = s IFFT(w (.) FFT(in)), one read and one write of HBM per point.
//
// Pow2Kernel's last pass leaves output element jof<NP-1>(t, q) + r N / R_last in v[q R_last + r]; its first pass wants input element jof<0>(t, q) + r N / R_0 in
// v[q R_0 + r].  Run the inverse transform with the radix list REVERSED and the two coincide: the forward transform's output registers are the inverse's input
// registers, so the product with w needs no exchange and no memory traffic but w itself (<= 64 KiB, L2-resident; the Rader kernel's pointwise product works the
// same way, rader_kernel.h).  The inverse's last pass then stores in the forward's load pattern.  IFFT(y) = conj(FFT(conj(y))): both pass sets are forward ones.
//
// The struct is two Pow2Kernel instantiations over the same (T, N, TPL, LPB, HALF, FLAGS, NT, VEC) and uses their passes<0> only.  Instantiated and launched
// from kernels_filter.hip (launch_filter).  FilterColKernel (below FilterKernel) is the same on a tile of ADJACENT lanes along a strided axis, staged through LDS (ColTile).
//
// REAL: the same on a REAL lane of n = 2N points under an R2C plan (MODE = FILTER_R2C): out = s IRFFT(w (.) RFFT(in)), w of N + 1 complex values.  The lane is
// read as N complex points z[m] = x[2m] + i x[2m+1] -- the load and the store are the complex kernel's, each complex element two adjacent reals -- and only the step
// between the two pass sets differs: the half spectrum X[k], X[N-k] of the real lane needs Z[k] AND Z[N-k], which another thread holds, so the lane goes through
// its LDS once more (write Z, barrier, gather the mirror bin; the components one after the other where the exchange buffer holds one), and every thread then
// splits, weights and folds its own bins in registers:
//   A = Z[k], B = conj Z[(N-k) mod N], W = e^{-2 pi i k/n}:   X[k] = (A+B)/2 + W (A-B)/(2i),   X[N-k] = conj((A+B)/2 - W (A-B)/(2i))       (k = 0: X[N] is the Nyquist bin)
//   Yk = w[k] X[k], Ym = w[N-k] X[N-k]  (k = 0: both lose their imaginary parts, as ndifft_r2c drops those of DC and Nyquist),   Z'[k] = (Yk + conj Ym) + i conj(W) (Yk - conj Ym)
// The unnormalised inverse FFT_N of Z' is y[2m] + i y[2m+1] with y = n irfft(w (.) rfft(x)).  Both bins of a pair are computed by both threads that hold one of
// them: twice the arithmetic of the split, no second exchange.
//
// FILTER_DCT: the same on a REAL lane of n = 2N points under a DCT plan (MODE = FILTER_DCT): out = s DCT3(g (.) DCT2(in)), g of n REAL values, both transforms the
// unnormalised lane definitions C[k] = sum_j x[j] cos(pi (2j+1) k / (2n)),  y[j] = D[0] / 2 + sum_{k>=1} D[k] cos(pi (2j+1) k / (2n))  (Makhoul; realops.h G_DCT2_EVEN,
// G_DCT3_EVEN).  With v[m] = x[2m], v[n-1-m] = x[2m+1] and V = RFFT_n(v), C[k] = Re(c_k V[k]), C[n-k] = -Im(c_k V[k]), c_k = e^{-i pi k/(2n)}; backwards
// V'[k] = conj(c_k) (D[k] - i D[n-k]) / 2 (D[n] := 0), v' = n irfft(V'), y[2m] = v'[m], y[2m+1] = v'[n-1-m].  The kernel:
//   load     the lane CONTIGUOUSLY (any base, any pitch: the accesses are sizeof(T) wide, or 16 bytes where the host found both sides aligned), through the lane's LDS
//            into z[m] = v[2m] + i v[2m+1] = x[4m] + i x[4m+2] (m < N/2), x[2n-1-4m] + i x[2n-3-4m] (m >= N/2) in the registers jof<0> names.  Element j of the lane
//            sits at slot(j): its class (j mod 4) block, position j / 4 -- both gathers then run at unit stride; where the exchange buffer holds one component (HALF)
//            the even elements go through first (the z of m < N/2), then the odd ones
//   mix      the real mode's exchange and split give V[k], V[N-k] (k = 0: V[0] and the Nyquist bin V[N]);  tk = c_k V[k], tm = c_{N-k} V[N-k];
//            D[k] = g[k] Re tk, D[n-k] = -g[n-k] Im tk (k = 0: 0), D[N-k] = g[N-k] Re tm, D[N+k] = -g[N+k] Im tm (k = 0: D[N] again);
//            V'[k], V'[N-k] as above, then herm_fold as in the real mode
//   store    z' = y[4m] + i y[4m+2] / y[2n-1-4m] + i y[2n-3-4m]: the load's map backwards through the LDS, contiguous global stores.  Dead tail lanes take part in
//            every staging barrier and store nothing; every load of a workgroup precedes its first barrier, so a call in place is safe.
#pragma once
#include <type_traits>
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
// The thread index behind a wall the optimiser does not see through.  The staged load and the staged store of the DCT form compute the SAME LDS addresses from t, 4 E of
// them; left alone the compiler computes them once and keeps them in registers across both pass sets (f64 F = 1024: 256 VGPRs + 7 AGPRs = one workgroup per CU; with
// the index laundered in front of each stage 220 = two.  profiles/r12/kernel_resources_filter_dct.txt)
__device__ __forceinline__ int opaque(int t) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));
#endif
    return t;
}
__device__ __forceinline__ void mix_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// The DCT pair mix loads W, two c and four g per bin (the real one W and two w).  0: no fence; 8: a fence behind EVERY bin (the last radix is 8 throughout).  Per instance,
// from the compiler's register counts (profiles/r12/kernel_resources_filter_dct.txt) and an A-B of two libraries built with NDFFT_FILTER_MIX_SPLIT = 0 / 8 on 2^24 points
// (profiles/r12/bench_filter_dct_fence_none.jsonl, _fence_all.jsonl; us without -> with):
//   f64  F = 64  71.9 -> 68.0 (120-140 -> 100-107 VGPRs),  F = 128  87.9 -> 75.2 (198 -> 165),  F = 512  87.8 -> 83.2 (140 -> 126),  F = 2048  124.4 -> 109.8 (same count)
//   f32  F = 64  44.6 -> 41.9 (78-88 -> 66-71),  F = 256  55.4 -> 52.4;  F = 1024 and the 4-byte form of F = 2048 by count alone (186 -> 145, 180 -> 156; times within 2 %)
// Every other instance is within 2 % either way and is left without, so that its loads overlap.
template <typename T, int N, int VEC> constexpr int filter_mix_split_dct() {
    if (NDFFT_FILTER_MIX_SPLIT >= 0) return NDFFT_FILTER_MIX_SPLIT;
    if (sizeof(T) == 8) return N == 64 || N == 128 || N == 512 || N == 2048 ? 8 : 0;
    return N == 64 || N == 256 || N == 1024 || (N == 2048 && VEC == 1) ? 8 : 0;
}

// MODE: FILTER_C2C / FILTER_R2C / FILTER_DCT of engine.h (a bool before the DCT form: false / true still name the first two)
// FILTER_DCT: VEC is the number of REALS per global access (1, or 16 / sizeof(T)); the pass sets always own butterflies j = t + q TPL
template <typename T, int V> struct real_vec { typedef T type __attribute__((ext_vector_type(V))); };

template <typename T, int N, int TPL, int LPB, bool HALF, typename RL, int FLAGS, int NT, int VEC, int MODE = FILTER_C2C> struct FilterKernel {
    static constexpr bool REAL = MODE == FILTER_R2C, DCT = MODE == FILTER_DCT, MIRROR = REAL || DCT;
    using RLR = typename Reversed<RL>::type;
    using KF = Pow2Kernel<T, N, TPL, LPB, HALF, RL, FLAGS, 1, NT, DCT ? 1 : VEC>;
    using KI = Pow2Kernel<T, N, TPL, LPB, HALF, RLR, FLAGS, 1, NT, DCT ? 1 : VEC>;
    static constexpr int E = KF::E, THREADS = KF::THREADS, NP = RL::NP, MIX_SPLIT = DCT ? filter_mix_split_dct<T, N, VEC>() : filter_mix_split<T, N>();
    static constexpr size_t LDS_BYTES = KF::LDS_BYTES;
    static constexpr int R0 = RL::at(0), NB0 = N / R0, NBF0 = KF::slots(0);                  // first pass of the forward list = last pass of the reversed one
    static constexpr int RZ = RL::at(NP - 1), NBZ = N / RZ, NBFZ = KF::slots(NP - 1);        // last pass of the forward list = first pass of the reversed one
    static_assert(KI::E == E && E * TPL == N, "both lists run whole butterfly rounds on the same registers");
    static_assert(KF::full(0) && KF::full(NP - 1), "whole rounds in the first and last pass");
    static_assert(DCT || VEC == 1 || (NBF0 % 2 == 0 && NBFZ % 2 == 0), "VEC = 2 needs an even number of butterfly rounds in the first and last pass");
    static_assert(MIX_SPLIT == 0 || RZ % MIX_SPLIT == 0, "a fence behind every RZ / MIX_SPLIT bins");
    static_assert(!DCT || (R0 % 2 == 0 && (2 * E) % VEC == 0 && N % 4 == 0 && (VEC == 1 || VEC * sizeof(T) == 16)), "DCT: whole accesses per thread; r < R0 / 2 names the z of m < N / 2");

    // FILTER_DCT staging.  Register x[i VEC + e] of thread t is element xj(t, i, e) of the lane: access i of a thread is the VEC reals from (t + i TPL) VEC on
    static constexpr int NX = 2 * E, NA = NX / VEC, ROUNDS = HALF ? 2 : 1, ODD0 = HALF ? 0 : N;
    static __device__ __forceinline__ int xj(int t, int i, int e) { return (t + i * TPL) * VEC + e; }
    // where element j waits in the lane's LDS, in reals: [odd j: a second half of the buffer, unless the odd elements have a round of their own] [bit 1 of j: N / 2] [j / 4]
    static __device__ __forceinline__ int slot(int j) { return phi((HALF ? 0 : (j & 1) * N) + ((j >> 1) & 1) * (N / 2) + (j >> 2)); }
    // z[m] <-> (lane elements, as slots): m < N / 2: x[4m], x[4m+2];  m >= N / 2, p = N - 1 - m: x[4p+3], x[4p+1]
    static __device__ __forceinline__ void stage_in(const T (&x)[NX], cpx<T> (&v)[E], char *lds, int t0) {
        T *s = (T *)lds;
        const int t = opaque(t0);
#pragma unroll
        for (int h = 0; h < ROUNDS; ++h) {
            if (h) __syncthreads();            // the first round's gathers are done
#pragma unroll
            for (int i = 0; i < NA; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int j = xj(t, i, e);
                    if (!HALF || (j & 1) == h) s[slot(j)] = x[i * VEC + e];
                }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NBF0; ++q)
#pragma unroll
                for (int r = 0; r < R0; ++r) {
                    const int m = KF::template jof<0>(t, q) + r * NB0, p = N - 1 - m;
                    if (r < R0 / 2) { if (!HALF || h == 0) v[q * R0 + r] = mk<T>(s[phi(m)], s[phi(N / 2 + m)]); }
                    else if (!HALF || h == 1) v[q * R0 + r] = mk<T>(s[phi(ODD0 + N / 2 + p)], s[phi(ODD0 + p)]);
                }
        }
    }
    static __device__ __forceinline__ void stage_out(const cpx<T> (&v)[E], T (&x)[NX], char *lds, int t0) {
        T *s = (T *)lds;
        const int t = opaque(t0);
#pragma unroll
        for (int h = 0; h < ROUNDS; ++h) {
            __syncthreads();                   // no thread still gathers from the second pass set's last exchange, or from the first round
#pragma unroll
            for (int q = 0; q < NBF0; ++q)
#pragma unroll
                for (int r = 0; r < R0; ++r) {
                    const int m = KI::template jof<NP - 1>(t, q) + r * NB0, p = N - 1 - m;
                    const cpx<T> z = v[q * R0 + r];
                    if (r < R0 / 2) { if (!HALF || h == 0) { s[phi(m)] = z.x; s[phi(N / 2 + m)] = z.y; } }
                    else if (!HALF || h == 1) { s[phi(ODD0 + N / 2 + p)] = z.x; s[phi(ODD0 + p)] = z.y; }
                }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NA; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int j = xj(t, i, e);
                    if (!HALF || (j & 1) == h) x[i * VEC + e] = s[slot(j)];
                }
        }
    }
    static_assert((FLAGS & ~16) == 0, "product flags other than the derived twiddle powers have no meaning here");

    // The steps between the two pass sets as functions of VALUES: a helper that takes the register arrays by reference moved the registers or the schedule of some
    // instance (profiles/r14/isa_diff.txt), so the loops over the registers, the loads, the stores and the DCT mix stay in run().
    // after the first pass set v[q RZ + r] of thread t is bin bin(t, q, r) of the lane's spectrum (the last pass's output index, pow2_kernel.h)
    static __device__ __forceinline__ int bin(int t, int q, int r) { return KF::template jof<NP - 1>(t, q) + r * NBZ; }
    // the pair split.  A = Z[k], B = conj Z[(N-k) mod N]:  e = (A + B) / 2,  o = W (A - B) / (2i)
    static __device__ __forceinline__ cpx<T> split_even(const cpx<T> A, const cpx<T> B) { return mk<T>((A.x + B.x) * (T)0.5, (A.y + B.y) * (T)0.5); }
    static __device__ __forceinline__ cpx<T> split_odd(const cpx<T> A, const cpx<T> B, const cpx<T> W) { return cmul(mk<T>((A.y - B.y) * (T)0.5, -(A.x - B.x) * (T)0.5), W); }
    // One bin's step: A = Z[k] in, conj(Z'[k]) out (the inverse runs forward passes); zm = Z[(N - k) mod N] from the mirror exchange.  The tables are read with the
    // default cache policy: every lane reads the same vectors.
    // C2C: the bin times its weight
    static __device__ __forceinline__ cpx<T> mix_c2c(const cpx<T> A, int k, const cpx<T> *w) { return cconj(cmul(A, w[k])); }
    // R2C pair mix (the formulas at the top; r2c_split_pair and herm_fold of realops.h on registers).  w: N + 1 values; wn[k] = W_n^k, k <= N
    static __device__ __forceinline__ cpx<T> mix_r2c(const cpx<T> A, const cpx<T> zm, int k, const cpx<T> *w, const cpx<T> *wn) {
        const cpx<T> W = wn[k], B = cconj(zm), e = split_even(A, B), o = split_odd(A, B, W);
        cpx<T> yk = cmul(w[k], cadd(e, o)), ym = cmul(w[N - k], cconj(csub(e, o)));
        if (k == 0) { yk.y = (T)0; ym.y = (T)0; }
        return herm_fold<T>(yk, cconj(ym), W);
    }

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
        if constexpr (DCT) {
            const T *xin = (const T *)a.in + (live ? lane : 0) * a.pitch_in;      // (pitches in reals)
            T x[NX];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                if constexpr (VEC == 1) {
                    if constexpr ((NT & 2) != 0) x[i] = __builtin_nontemporal_load(xin + xj(t, i, 0)); else x[i] = xin[xj(t, i, 0)];
                } else {
                    typedef typename real_vec<T, VEC>::type XV;
                    XV w;
                    if constexpr ((NT & 2) != 0) w = __builtin_nontemporal_load((const XV *)(xin + xj(t, i, 0))); else w = *(const XV *)(xin + xj(t, i, 0));
#pragma unroll
                    for (int e = 0; e < VEC; ++e) x[i * VEC + e] = w[e];
                }
            }
            stage_in(x, v, lds, t);
        } else if constexpr (VEC == 2) {
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
        // v[q RZ + r] is bin(t, q, r): mixed with its weight(s), conjugated for the inverse
        if constexpr (!MIRROR) {
            const cpx<T> *w = (const cpx<T> *)f.w;
#pragma unroll
            for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                for (int r = 0; r < RZ; ++r) v[q * RZ + r] = mix_c2c(v[q * RZ + r], bin(t, q, r), w);
        } else {
            // mirror exchange: b[i] = Z[(N - k) mod N] for the bin k of v[i], through the lane's LDS: whole elements in one round, or the components one after the other
            // where the exchange buffer holds one (HALF).  The barrier in front of a write: no thread still reads what the write replaces (the last exchange of the
            // first pass set, the other component's round); dead tail lanes take part in every barrier
            cpx<T> b[E];
            using S = typename std::conditional<HALF, T, cpx<T>>::type;      // what one round moves
            S *s = (S *)lds;
#pragma unroll
            for (int half = 0; half < (HALF ? 2 : 1); ++half) {
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) {
                        if constexpr (HALF) s[phi(bin(t, q, r))] = half ? v[q * RZ + r].y : v[q * RZ + r].x; else s[phi(bin(t, q, r))] = v[q * RZ + r];
                    }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) {
                        const S x = s[phi((N - bin(t, q, r)) & (N - 1))];
                        if constexpr (HALF) { if (half) b[q * RZ + r].y = x; else b[q * RZ + r].x = x; } else b[q * RZ + r] = x;
                    }
            }
            if constexpr (DCT) {
                // pair mix (the formulas at the top).  g: 2 N reals, c[k] = e^{-i pi k/(4N)}, k < 2 N, wn[k] = W_n^k, k <= N: default cache policy, every lane reads the same
                const T *g = (const T *)f.w;
                const cpx<T> *wn = (const cpx<T> *)f.wn, *c = (const cpx<T> *)f.c;
                const T hf = (T)0.5;
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) {
                        const int k = bin(t, q, r);
                        const cpx<T> A = v[q * RZ + r], B = cconj(b[q * RZ + r]), W = wn[k], ck = c[k], cm = c[N - k];
                        const cpx<T> e = split_even(A, B), o = split_odd(A, B, W);
                        const cpx<T> tk = cmul(ck, cadd(e, o)), tm = cmul(cm, cconj(csub(e, o)));                  // c_k V[k], c_{N-k} V[N-k]
                        const T dk = hf * g[k] * tk.x, dm = hf * g[N - k] * tm.x;                                    // D[k] / 2, D[N-k] / 2
                        const T dnk = k ? -hf * g[(2 * N - k) & (2 * N - 1)] * tk.y : (T)0, dpk = k ? -hf * g[N + k] * tm.y : dm;     // D[n-k] / 2 (D[n] := 0; g has no element n), D[N+k] / 2 (k = 0: D[N] once)
                        const cpx<T> vk = cmul(cconj(ck), mk<T>(dk, -dnk)), vm = cmul(cconj(cm), mk<T>(dm, -dpk));   // V'[k], V'[N-k]
                        v[q * RZ + r] = herm_fold<T>(vk, cconj(vm), W);      // conj(Z'[k]): the inverse runs forward passes
                        if constexpr (MIX_SPLIT > 0) { if ((r + 1) % (RZ / MIX_SPLIT) == 0) mix_fence(); }
                    }
            } else {
                const cpx<T> *w = (const cpx<T> *)f.w, *wn = (const cpx<T> *)f.wn;
#pragma unroll
                for (int q = 0; q < NBFZ; ++q)
#pragma unroll
                    for (int r = 0; r < RZ; ++r) {
                        v[q * RZ + r] = mix_r2c(v[q * RZ + r], b[q * RZ + r], bin(t, q, r), w, wn);
                        if constexpr (MIX_SPLIT > 0) { if ((r + 1) % (RZ / MIX_SPLIT) == 0) mix_fence(); }
                    }
            }
        }
        // (the first exchange of the second pass set starts with a barrier: no thread overwrites LDS another still reads from the first set's last exchange, or gathers from)
        KI::template passes<0>(v, (const cpx<T> *)f.twp_rev, lds, t);
        if constexpr (!DCT) { if (!live) return; }
        const T sc = (T)a.scale;
#pragma unroll
        for (int i = 0; i < E; ++i) { v[i].x *= sc; v[i].y *= -sc; }
        if constexpr (DCT) {
            T x[NX];
            stage_out(v, x, lds, t);
            if (!live) return;
            T *xout = (T *)a.out + lane * a.pitch_out;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                if constexpr (VEC == 1) {
                    if constexpr ((NT & 1) != 0) __builtin_nontemporal_store(x[i], xout + xj(t, i, 0)); else xout[xj(t, i, 0)] = x[i];
                } else {
                    typedef typename real_vec<T, VEC>::type XV;
                    XV w;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) w[e] = x[i * VEC + e];
                    if constexpr ((NT & 1) != 0) __builtin_nontemporal_store(w, (XV *)(xout + xj(t, i, 0))); else *(XV *)(xout + xj(t, i, 0)) = w;
                }
            }
        } else if constexpr (VEC == 2) {
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

// ---- column form: the transform axis is strided and ADJACENT LANES are contiguous (any axis but the last of a C-layout array) -----------------------------------
// ColTile: a tile of LPB adjacent lanes x NE elements of type S between global memory and the workgroup's LDS, lanes fastest on the global side -- the staging of
// RealPow2Kernel<..., COL = true> (pow2_real.h) on its own, so that the column forms of the real and cosine filters can use it with S = T.  Thread -> (cl = tid % LPB
// fastest, row j0 = tid / LPB); rows j0, j0 + STEP, ... of the tile go to lane cl's slice of PITCH elements, PITCH odd: adjacent lanes fall on different banks.
template <bool NT, typename S> __device__ __forceinline__ S tile_load(const S *p) {
    if constexpr (!NT) return *p;
    else if constexpr (std::is_same<S, cpx<double>>::value) return gload<double, true>(p);
    else return __builtin_nontemporal_load(p);
}
template <bool NT, typename S> __device__ __forceinline__ void tile_store(S *p, S v) {
    if constexpr (!NT) *p = v;
    else if constexpr (std::is_same<S, cpx<double>>::value) gstore<double, true>(p, v);
    else __builtin_nontemporal_store(v, p);
}
template <typename S, int NE, int LPB, int THREADS, int PITCH> struct ColTile {
    static constexpr int STEP = THREADS / LPB, PER = NE / STEP;
    static_assert(THREADS % LPB == 0 && NE % STEP == 0, "whole rows of the tile per round, whole rounds per lane");
    static_assert(PITCH % 2 == 1 && PITCH >= NE, "an odd slice pitch that holds the lane");
    static constexpr size_t LDS_BYTES = (size_t)LPB * PITCH * sizeof(S);
    // this thread's lane in the load / store role: element 0 of it on both sides (in S), its slice; dead = past the last lane of a ragged last tile
    struct Pos { int j0; bool live; int64_t in, out; S *slice; };
    static __device__ __forceinline__ Pos pos(const FilterArgs &f, int64_t lane0, char *smem) {
        Pos p;
        const int cl = threadIdx.x % LPB;
        p.j0 = threadIdx.x / LPB;
        const int64_t L = lane0 + cl;
        p.live = L < f.a.nlanes;
        int64_t o, i;
        if (f.a.nlanes <= 0x7fffffffLL) {      // (inner <= nlanes: both fit 32 bits, and a 64-bit division is about 60 VALU instructions per thread)
            const uint32_t l = p.live ? (uint32_t)L : 0u, in = (uint32_t)f.inner;
            o = l / in; i = l % in;
        } else {
            const int64_t l = p.live ? L : 0;
            o = l / f.inner; i = l % f.inner;
        }
        p.in = o * f.outer_in + i; p.out = o * f.outer_out + i;
        p.slice = (S *)smem + (size_t)cl * PITCH;
        return p;
    }
    // every global load of the tile, into registers: nothing is stored to LDS, and no barrier passed, before the last one is issued
    template <bool NT> static __device__ __forceinline__ void load(const Pos &p, const S *in, int64_t elem, S (&x)[PER]) {
        if (p.live) {
            const S *src = in + p.in + (int64_t)p.j0 * elem;
#pragma unroll
            for (int i = 0; i < PER; ++i) x[i] = tile_load<NT>(src + (int64_t)(i * STEP) * elem);
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) x[i] = S{};
        }
    }
    static __device__ __forceinline__ void put(const Pos &p, const S (&x)[PER]) {
#pragma unroll
        for (int i = 0; i < PER; ++i) p.slice[p.j0 + i * STEP] = x[i];
    }
    // the tile back, lanes fastest; a dead lane stores nothing
    template <bool NT> static __device__ __forceinline__ void store(const Pos &p, S *out, int64_t elem) {
        if (!p.live) return;
        S *dst = out + p.out + (int64_t)p.j0 * elem;
#pragma unroll
        for (int i = 0; i < PER; ++i) tile_store<NT>(dst + (int64_t)(i * STEP) * elem, p.slice[p.j0 + i * STEP]);
    }
};

// FilterColKernel: FilterKernel's FILTER_C2C on a column tile.  load (ColTile, every global load of the workgroup ahead of its first barrier: a tile is whole lanes and
// tiles are disjoint, so a call in place is safe) | barrier | threads change role to (t = tid % TPL, ll = tid / TPL) and gather v[q R0 + r] = slice[jof<0>(t, q) + r N / R0]
// | forward passes, mix_c2c, reversed passes, scale and conjugate as in the row form, the lane's slice the exchange buffer | barrier | scatter to the slice at
// jof<NP-1> | barrier | store.  Dead lanes of a ragged last tile are zeros, take part in every barrier and store nothing.
// HALF: the slice holds whole complex elements either way, so the component-wise exchange saves no LDS here, only doubles the exchange's barriers and LDS instructions;
// the instances run whole elements (kernels_filter.hip), as the column transforms of pow2_real.h do.
template <typename T, int N, int TPL, int LPB, bool HALF, typename RL, int FLAGS, int NT, int MODE = FILTER_C2C> struct FilterColKernel {
    static_assert(MODE == FILTER_C2C, "the column forms of the real and cosine filters are not written yet");
    using RLR = typename Reversed<RL>::type;
    using KF = Pow2Kernel<T, N, TPL, LPB, HALF, RL, FLAGS, 1, NT, 1>;
    using KI = Pow2Kernel<T, N, TPL, LPB, HALF, RLR, FLAGS, 1, NT, 1>;
    static constexpr int E = KF::E, THREADS = KF::THREADS, NP = RL::NP;
    static constexpr int PITCH = (N + (N >> 4) + 2) | 1;      // RealPow2Kernel::LANE_LDS for COL
    using Tile = ColTile<cpx<T>, N, LPB, THREADS, PITCH>;
    static constexpr size_t LDS_BYTES = Tile::LDS_BYTES;
    static constexpr int R0 = RL::at(0), NB0 = N / R0, NBF0 = KF::slots(0);
    static constexpr int RZ = RL::at(NP - 1), NBZ = N / RZ, NBFZ = KF::slots(NP - 1);
    static_assert(KI::E == E && E * TPL == N && Tile::PER == E && Tile::STEP == TPL, "both lists run whole butterfly rounds on the same registers; the load fills them once");
    static_assert(KF::full(0) && KF::full(NP - 1), "whole rounds in the first and last pass");
    static_assert(PITCH >= KF::LANE_LDS, "the slice is the lane's exchange buffer");
    static_assert((FLAGS & ~16) == 0, "product flags other than the derived twiddle powers have no meaning here");

    static __device__ __forceinline__ void run(const FilterArgs &f) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        const Pow2Args &a = f.a;
        const int64_t lane0 = (int64_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_chunk) * LPB;
        const typename Tile::Pos p = Tile::pos(f, lane0, smem);
        cpx<T> v[E];
        Tile::template load<(NT & 2) != 0>(p, (const cpx<T> *)a.in, f.elem_in, v);
        Tile::put(p, v);
        __syncthreads();
        const int t = threadIdx.x % TPL, ll = threadIdx.x / TPL;
        cpx<T> *slice = (cpx<T> *)smem + (size_t)ll * PITCH;
#pragma unroll
        for (int q = 0; q < NBF0; ++q)
#pragma unroll
            for (int r = 0; r < R0; ++r) v[q * R0 + r] = slice[KF::template jof<0>(t, q) + r * NB0];
        // (the first exchange of a pass set starts with a barrier: every gather above, and of the first set's last exchange, is done before a slice is overwritten)
        KF::template passes<0>(v, (const cpx<T> *)a.twp, (char *)slice, t);
        const cpx<T> *w = (const cpx<T> *)f.w;
#pragma unroll
        for (int q = 0; q < NBFZ; ++q)
#pragma unroll
            for (int r = 0; r < RZ; ++r) {
                const int k = KF::template jof<NP - 1>(t, q) + r * NBZ;      // FilterKernel::bin
                v[q * RZ + r] = cconj(cmul(v[q * RZ + r], w[k]));           // FilterKernel::mix_c2c
            }
        KI::template passes<0>(v, (const cpx<T> *)f.twp_rev, (char *)slice, t);
        const T sc = (T)a.scale;
#pragma unroll
        for (int i = 0; i < E; ++i) { v[i].x *= sc; v[i].y *= -sc; }
        __syncthreads();      // no thread still gathers from the second set's last exchange
#pragma unroll
        for (int q = 0; q < NBF0; ++q)
#pragma unroll
            for (int r = 0; r < R0; ++r) slice[KI::template jof<NP - 1>(t, q) + r * NB0] = v[q * R0 + r];
        __syncthreads();
        Tile::template store<(NT & 1) != 0>(p, (cpx<T> *)a.out, f.elem_out);
    }
};

template <typename K> __global__ __launch_bounds__(K::THREADS, 1) void k_filter_pow2(const FilterArgs f) { K::run(f); }

}  // namespace ndfft
