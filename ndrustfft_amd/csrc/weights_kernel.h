// weights_kernel.h -- the diagonal normalisation pass (Normalization::Weights): dst[lane, j] = src[lane, j] * w[j] over the lanes of an
// n-d view, for real and complex elements of f32 / f64 (complex x complex: the full product).  One pass over the array, at the point
// where the reference would call a custom normalisation function: before the transform (C2R, DCT-I..IV: caller's input -> a scratch
// image, cache-allocating stores, the transform reads it at once) or after it (C2C inverse: in place on the output view, streaming
// stores like the transform kernels' own outputs).  dst == src with identical geometry is legal: every element is read and written
// by the same thread, once.  Included by transpose.hip; launcher: launch_weights (engine.h).
//
// Three thread maps, chosen on the host (launch_weights):
//   row      axis stride 1 on both sides.  Consecutive threads take consecutive 16-byte vectors of a lane; a thread loads its slice
//            of w ONCE and walks a block of lanes with it (offsets by an odometer over the batch dims: a division only at a carry).
//   column   a batch dim with stride 1 on both sides.  Consecutive threads take consecutive lanes of that dim (16-byte vectors
//            along it); j comes from the block index and a loop counter only, so w[j] is one load per wave.
//   general  anything else (negative / stepped axis strides without a unit-stride batch dim): one element per thread, indexed.
// The 16-byte accesses need base pointers, pitches and (row form) w aligned to 16 bytes -- checked at launch; otherwise, and in the
// tail of a lane (row) / of the inner dim (column) whose length is no multiple of the vector, the accesses are one element wide.
#pragma once
#include "engine.h"

namespace ndfft {

// batch dims of the pass, slowest first, padded AT THE FRONT with shape 1 / stride 0 (the kernels never look at a dim count)
struct WGeom {
    int64_t sh[kMaxBatchDims], ss[kMaxBatchDims], ds[kMaxBatchDims];   // extents, strides of src / dst in ELEMENTS
};

// K scalars of type T moved by one access: K = 1 is the scalar itself
template <typename T, int K> struct WAcc { typedef T type __attribute__((ext_vector_type(K))); };
template <typename T> struct WAcc<T, 1> { typedef T type; };

// x * w for one access of K scalars: K reals, or K / 2 complex numbers {re, im}
template <typename T, int CPLX, int K>
__device__ __forceinline__ typename WAcc<T, K>::type wmul(typename WAcc<T, K>::type x, typename WAcc<T, K>::type w) {
    if constexpr (!CPLX) {
        return x * w;
    } else {
        typename WAcc<T, K>::type r;
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            r[k] = x[k] * w[k] - x[k + 1] * w[k + 1];
            r[k + 1] = x[k] * w[k + 1] + x[k + 1] * w[k];
        }
        return r;
    }
}
// one element (C scalars) repeated over an access of K scalars
template <typename T, int C, int K>
__device__ __forceinline__ typename WAcc<T, K>::type wsplat(typename WAcc<T, C>::type e) {
    if constexpr (K == C) {
        return e;
    } else if constexpr (C == 1) {
        typename WAcc<T, K>::type r;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = e;
        return r;
    } else {
        typename WAcc<T, K>::type r;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = e[k % C];
        return r;
    }
}
template <int NT, typename A> __device__ __forceinline__ void wstore(A v, A *p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// offsets of lane L and of the lanes after it.  Coordinates of dims 1..3 only: dim 0 is the slowest and never carries out.
struct WWalk {
    int64_t c1, c2, c3, so, dof;
    __device__ __forceinline__ void init(const WGeom &g, int64_t lane) {
        c3 = lane % g.sh[3]; lane /= g.sh[3];
        c2 = lane % g.sh[2]; lane /= g.sh[2];
        c1 = lane % g.sh[1]; lane /= g.sh[1];
        so = lane * g.ss[0] + c1 * g.ss[1] + c2 * g.ss[2] + c3 * g.ss[3];
        dof = lane * g.ds[0] + c1 * g.ds[1] + c2 * g.ds[2] + c3 * g.ds[3];
    }
    __device__ __forceinline__ void step(const WGeom &g, int64_t s) {   // s lanes further
        c3 += s; so += s * g.ss[3]; dof += s * g.ds[3];
        if (c3 >= g.sh[3]) {
            const int64_t q = c3 / g.sh[3];
            c3 -= q * g.sh[3]; c2 += q;
            so += q * (g.ss[2] - g.sh[3] * g.ss[3]); dof += q * (g.ds[2] - g.sh[3] * g.ds[3]);
            if (c2 >= g.sh[2]) {
                const int64_t q2 = c2 / g.sh[2];
                c2 -= q2 * g.sh[2]; c1 += q2;
                so += q2 * (g.ss[1] - g.sh[2] * g.ss[2]); dof += q2 * (g.ds[1] - g.sh[2] * g.ds[2]);
                if (c1 >= g.sh[1]) {
                    const int64_t q3 = c1 / g.sh[1];
                    c1 -= q3 * g.sh[1];
                    so += q3 * (g.ss[0] - g.sh[1] * g.ss[1]); dof += q3 * (g.ds[0] - g.sh[1] * g.ds[1]);
                }
            }
        }
    }
};

// lanes [first, first + count * step) in steps of `step`, element (vector) at j0 of each: four loads in flight, then four stores
// (src and dst may be the same array, so the compiler cannot move a load above a store by itself)
template <typename T, int CPLX, int K, int NT>
__device__ __forceinline__ void wrow_walk(const T *src, T *dst, const WGeom &g, typename WAcc<T, K>::type wv, int64_t j0, int64_t first,
                                          int64_t step, int count, int64_t nlanes) {
    typedef typename WAcc<T, K>::type A;
    constexpr int C = CPLX ? 2 : 1;
    WWalk wk;
    wk.init(g, first);
    int64_t lane = first;
    for (int k = 0; k < count; k += 4) {
        int64_t so[4], dof[4];
        bool ok[4];
        A x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = k + u < count && lane < nlanes;
            so[u] = wk.so; dof[u] = wk.dof;
            if (ok[u]) x[u] = *(const A *)(src + (so[u] + j0) * C);
            wk.step(g, step); lane += step;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) wstore<NT>(wmul<T, CPLX, K>(x[u], wv), (A *)(dst + (dof[u] + j0) * C));
    }
}

// row form.  Block = 2^tx_log threads along the lane x (256 >> tx_log) lanes at a time, lpt rounds of them; grid.x: vector blocks
// of the lane, grid.y: lane blocks (grid-stride).  K: scalars per access (16 bytes, or one element)
template <typename T, int CPLX, int K, int NT>
__global__ __launch_bounds__(256) void k_weights_row(const T *src, T *dst, const T *__restrict__ w, const WGeom g, int64_t nlanes, int64_t n,
                                                     int tx_log, int lpt) {
    constexpr int C = CPLX ? 2 : 1, EV = K / C;   // scalars per element, elements per access
    typedef typename WAcc<T, K>::type A;
    typedef typename WAcc<T, C>::type E1;
    const int tx = (int)threadIdx.x & ((1 << tx_log) - 1), ty = (int)threadIdx.x >> tx_log, nty = 256 >> tx_log;
    const int64_t j0 = ((((int64_t)blockIdx.x) << tx_log) + tx) * EV;
    if (j0 >= n) return;
    const int64_t per_block = (int64_t)nty * lpt, nlb = (nlanes + per_block - 1) / per_block;
    if (j0 + EV <= n) {
        const A wv = *(const A *)(w + j0 * C);
        for (int64_t lb = blockIdx.y; lb < nlb; lb += gridDim.y)
            wrow_walk<T, CPLX, K, NT>(src, dst, g, wv, j0, lb * per_block + ty, nty, lpt, nlanes);
    } else {
        // the tail of a lane whose length is no multiple of the vector: element-wide
        for (int e = 0; e < EV - 1; ++e) {
            if (j0 + e >= n) break;
            const E1 we = *(const E1 *)(w + (j0 + e) * C);
            for (int64_t lb = blockIdx.y; lb < nlb; lb += gridDim.y)
                wrow_walk<T, CPLX, C, NT>(src, dst, g, we, j0 + e, lb * per_block + ty, nty, lpt, nlanes);
        }
    }
}

// column form.  g: the OUTER batch dims (everything but the unit-stride one, `inner` long); block = 2^tx_log threads along the inner
// dim x (256 >> tx_log) outer indices; grid.x: vector blocks of the inner dim, grid.y: blocks of jb consecutive j (grid-stride),
// grid.z: blocks of outer indices (grid-stride).  xs / ys: axis strides.
template <typename T, int CPLX, int K, int NT>
__global__ __launch_bounds__(256) void k_weights_col(const T *src, T *dst, const T *__restrict__ w, const WGeom g, int64_t nouter, int64_t inner,
                                                     int64_t n, int64_t xs, int64_t ys, int tx_log, int jb) {
    constexpr int C = CPLX ? 2 : 1, EV = K / C;
    typedef typename WAcc<T, K>::type A;
    typedef typename WAcc<T, C>::type E1;
    const int tx = (int)threadIdx.x & ((1 << tx_log) - 1), ty = (int)threadIdx.x >> tx_log, nty = 256 >> tx_log;
    const int64_t i0 = ((((int64_t)blockIdx.x) << tx_log) + tx) * EV;
    if (i0 >= inner) return;
    const bool full = i0 + EV <= inner;
    const int64_t njb = (n + jb - 1) / jb, nob = (nouter + nty - 1) / nty;
    for (int64_t ob = blockIdx.z; ob < nob; ob += gridDim.z) {
        const int64_t o = ob * nty + ty;
        if (o >= nouter) continue;
        WWalk wk;
        wk.init(g, o);
        for (int64_t b = blockIdx.y; b < njb; b += gridDim.y) {
            const int64_t jlo = b * jb, jhi = jlo + jb < n ? jlo + jb : n;
            for (int64_t j = jlo; j < jhi; ++j) {
                const E1 we = *(const E1 *)(w + j * C);   // uniform over the block
                const T *s = src + (wk.so + j * xs + i0) * C;
                T *d = dst + (wk.dof + j * ys + i0) * C;
                if (full) {
                    wstore<NT>(wmul<T, CPLX, K>(*(const A *)s, wsplat<T, C, K>(we)), (A *)d);
                } else {
                    for (int e = 0; e < EV - 1; ++e)
                        if (i0 + e < inner) wstore<NT>(wmul<T, CPLX, C>(*(const E1 *)(s + e * C), we), (E1 *)(d + e * C));
                }
            }
        }
    }
}

// general form: one element per thread, plain indexed (grid-stride)
template <typename T, int CPLX, int NT>
__global__ __launch_bounds__(256) void k_weights_any(const T *src, T *dst, const T *__restrict__ w, const WGeom g, int64_t nlanes, int64_t n,
                                                     int64_t xs, int64_t ys) {
    constexpr int C = CPLX ? 2 : 1;
    typedef typename WAcc<T, C>::type E1;
    const int64_t total = nlanes * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t lane = i / n, j = i - lane * n;
        WWalk wk;
        wk.init(g, lane);
        const E1 x = *(const E1 *)(src + (wk.so + j * xs) * C);
        wstore<NT>(wmul<T, CPLX, C>(x, *(const E1 *)(w + j * C)), (E1 *)(dst + (wk.dof + j * ys) * C));
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr unsigned kWeightsMaxGridYZ = 32768;   // grid.y / grid.z stay below the limit of 65535; the kernels stride over the rest

template <typename T, int CPLX, int NT>
static int launch_weights_t(const T *src, T *dst, const T *w, const LaneGeom &gs, const LaneGeom &gd, int64_t n, hipStream_t s) {
    constexpr int C = CPLX ? 2 : 1;
    constexpr int KV = 16 / (int)sizeof(T);                 // scalars per 16-byte access
    constexpr int EV = KV / C;                              // elements per 16-byte access (1 for complex f64: the element IS the vector)
    constexpr size_t esz = sizeof(T) * C;
    // batch dims of the pass: extent-1 dims and dims that are broadcast on BOTH sides (stride 0: one image serves every index) dropped
    struct Dim { int64_t sh, ss, ds; };
    Dim dims[kMaxBatchDims];
    int nd = 0;
    if (gs.nb != gd.nb || gs.nb > kMaxBatchDims) return fail(NDFFT_ERR_INVALID_ARG, "internal: weight pass geometry");
    for (int i = 0; i < gs.nb; ++i) {
        if (gs.bshape[i] != gd.bshape[i]) return fail(NDFFT_ERR_INVALID_ARG, "internal: weight pass geometry");
        if (gs.bshape[i] == 1 || (gs.bstride[i] == 0 && gd.bstride[i] == 0)) continue;
        dims[nd++] = {gs.bshape[i], gs.bstride[i], gd.bstride[i]};
    }
    int64_t nlanes = 1;
    for (int i = 0; i < nd; ++i) nlanes *= dims[i].sh;
    if (nlanes <= 0 || n <= 0) return NDFFT_OK;
    const int64_t xs = n == 1 ? 1 : gs.axis_stride, ys = n == 1 ? 1 : gd.axis_stride;
    auto pack = [&](WGeom &g, int skip) {
        int m = 0;
        for (int i = 0; i < nd; ++i) m += i != skip;
        int at = kMaxBatchDims - m;
        for (int i = 0; i < at; ++i) { g.sh[i] = 1; g.ss[i] = 0; g.ds[i] = 0; }
        for (int i = 0; i < nd; ++i) if (i != skip) { g.sh[at] = dims[i].sh; g.ss[at] = dims[i].ss; g.ds[at] = dims[i].ds; ++at; }
    };
    auto aligned = [&](int skip, bool axis_too) {   // every pitch but the unit-stride one, and both base pointers, on 16 bytes
        if ((uintptr_t)src % 16 || (uintptr_t)dst % 16) return false;
        for (int i = 0; i < nd; ++i) if (i != skip && ((dims[i].ss * (int64_t)esz) % 16 || (dims[i].ds * (int64_t)esz) % 16)) return false;
        if (axis_too && ((xs * (int64_t)esz) % 16 || (ys * (int64_t)esz) % 16)) return false;
        return true;
    };
    WGeom g;
    if (xs == 1 && ys == 1) {
        pack(g, -1);
        const bool vec = EV > 1 && n >= EV && aligned(-1, false) && (uintptr_t)w % 16 == 0;
        const int64_t nvec = vec ? (n + EV - 1) / EV : n;
        int tx_log = 0;
        while ((1 << tx_log) < 256 && ((int64_t)1 << tx_log) < nvec) ++tx_log;
        const int nty = 256 >> tx_log;
        const int64_t gx = (nvec + (1 << tx_log) - 1) >> tx_log;
        int lpt = 16;                                          // lanes per thread; fewer while that leaves the device short of blocks
        while (lpt > 1 && gx * ((nlanes + (int64_t)nty * lpt - 1) / ((int64_t)nty * lpt)) < 2048) lpt >>= 1;
        const int64_t nlb = (nlanes + (int64_t)nty * lpt - 1) / ((int64_t)nty * lpt);
        const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(nlb, kWeightsMaxGridYZ), 1);
        if (vec) hipLaunchKernelGGL((k_weights_row<T, CPLX, KV, NT>), grid, dim3(256), 0, s, src, dst, w, g, nlanes, n, tx_log, lpt);
        else hipLaunchKernelGGL((k_weights_row<T, CPLX, C, NT>), grid, dim3(256), 0, s, src, dst, w, g, nlanes, n, tx_log, lpt);
        NDFFT_HIP(hipGetLastError());
        return NDFFT_OK;
    }
    int in = -1;
    for (int i = nd - 1; i >= 0; --i) if (dims[i].ss == 1 && dims[i].ds == 1) { in = i; break; }
    if (in >= 0) {
        pack(g, in);
        const int64_t inner = dims[in].sh, nouter = nlanes / inner;
        const bool vec = EV > 1 && inner >= EV && aligned(in, true);
        const int64_t nvec = vec ? (inner + EV - 1) / EV : inner;
        int tx_log = 0;
        while ((1 << tx_log) < 256 && ((int64_t)1 << tx_log) < nvec) ++tx_log;
        const int nty = 256 >> tx_log;
        const int64_t gx = (nvec + (1 << tx_log) - 1) >> tx_log, nob = (nouter + nty - 1) / nty;
        int jb = 16;
        while (jb > 1 && gx * nob * ((n + jb - 1) / jb) < 2048) jb >>= 1;
        const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>((n + jb - 1) / jb, kWeightsMaxGridYZ), (unsigned)std::min<int64_t>(nob, kWeightsMaxGridYZ));
        if (vec) hipLaunchKernelGGL((k_weights_col<T, CPLX, KV, NT>), grid, dim3(256), 0, s, src, dst, w, g, nouter, inner, n, xs, ys, tx_log, jb);
        else hipLaunchKernelGGL((k_weights_col<T, CPLX, C, NT>), grid, dim3(256), 0, s, src, dst, w, g, nouter, inner, n, xs, ys, tx_log, jb);
        NDFFT_HIP(hipGetLastError());
        return NDFFT_OK;
    }
    pack(g, -1);
    const unsigned grid = (unsigned)std::min<int64_t>((nlanes * n + 255) / 256, 16384);
    hipLaunchKernelGGL((k_weights_any<T, CPLX, NT>), dim3(grid), dim3(256), 0, s, src, dst, w, g, nlanes, n, xs, ys);
    NDFFT_HIP(hipGetLastError());
    return NDFFT_OK;
}

int launch_weights(const void *src, void *dst, const void *w, const LaneGeom &gs, const LaneGeom &gd, int64_t n, int dtype, int cplx,
                   int nt_store, hipStream_t s) {
#define NDFFT_W(T, CP, NT) launch_weights_t<T, CP, NT>((const T *)src, (T *)dst, (const T *)w, gs, gd, n, s)
    if (dtype == NDFFT_F32) return cplx ? (nt_store ? NDFFT_W(float, 1, 1) : NDFFT_W(float, 1, 0)) : (nt_store ? NDFFT_W(float, 0, 1) : NDFFT_W(float, 0, 0));
    return cplx ? (nt_store ? NDFFT_W(double, 1, 1) : NDFFT_W(double, 1, 0)) : (nt_store ? NDFFT_W(double, 0, 1) : NDFFT_W(double, 0, 0));
#undef NDFFT_W
}

}  // namespace ndfft
