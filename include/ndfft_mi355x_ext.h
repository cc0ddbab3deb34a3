/*
 * ndfft_mi355x_ext.h -- entry points added to libndfft_mi355x.so after the core header was frozen for its C99 consumers
 * (ABI minor 4: the weighted call; minor 5: the filter; minor 6: the DCT filter; minor 7: the kept share of a streamed input, in ndfft_mi355x_keep.h).  C99; includes ndfft_mi355x.h.
 *
 * Normalization::Weights(w): a DIAGONAL normalisation -- a different factor per element of the lane (orthonormal DCT
 * scalings, DCT-I end-point factors, spectral filters, de-aliasing masks).  Unlike Normalization::Custom(fn), a host
 * function that can never run on the GPU, a diagonal is a vector, and the vector lives in device memory.
 *
 * The weights multiply the lane element by element at the point where the reference would call the custom function, and like
 * Custom they REPLACE the default scaling (nothing is applied on top):
 *
 *   op                       where                                              weighted lane     d_weights
 *   NDFFT_OP_C2C_FWD, R2C    ignored (lib.rs:313-318, 497-503)                  --                may be NULL
 *   NDFFT_OP_C2C_INV         after, on the output lane (lib.rs:326-330)         n complex         n x Complex<T>
 *   NDFFT_OP_C2R             before, on the input lane; then Im(DC) and, for    n/2 + 1 complex   (n/2 + 1) x Complex<T>
 *                            even n, Im(Nyquist) are dropped (lib.rs:511-521)
 *   NDFFT_OP_DCT1..4         before, on the input lane (lib.rs:692-696)         n real            n x T
 *
 * Complex weights on complex lanes: the full complex product.
 */
#ifndef NDFFT_MI355X_EXT_H
#define NDFFT_MI355X_EXT_H

#include "ndfft_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ndfft_exec_device with Normalization::Weights.  Asynchronous on `stream`; the same argument checks, with the same panic texts in
 * the same order, as ndfft_exec_device.  d_weights: device memory of the element type in the table above, read on `stream`;
 * n_weights must equal the weighted lane's length (NDFFT_ERR_INVALID_ARG otherwise; the message names both numbers).  For the two
 * forward ops the weights are ignored and may be NULL; for every other op a NULL d_weights is NDFFT_ERR_INVALID_ARG.
 * C2R and DCT-I..IV weight the caller's input into a scratch image kept per host thread and stream (allocated by the first call of a
 * size: warm a shape up before capturing it into a HIP graph, as for every multi-pass route); C2C inverse weights the output view in
 * place, after the transform, and writes nothing outside it.  ndfft_last_path() reports "weights+<route>" / "<route>+weights".
 * A captured graph holds the scratch pointers of its (host thread, stream): a later larger multi-pass call by that thread on that stream,
 * ndfft_release_workspace and the thread's exit free them, and after any of the three the graph must be captured again (docs/streams.md). */
int ndfft_exec_weighted_device(const ndfft_plan *plan, int op, const void *d_in, void *d_out, int ndim,
                               const int64_t *shape_in, const int64_t *stride_in,
                               const int64_t *shape_out, const int64_t *stride_out,
                               int axis, const void *d_weights, size_t n_weights, void *stream);

/* ndfft_filter: for every lane along `axis`, out = s * IFFT(w (.) FFT(in)) -- exactly what ndfft -> lane *= w -> ndifft give under the normalisation `norm`
 * (s = 1 for NDFFT_NORM_NONE, 1 / n for NDFFT_NORM_DEFAULT, `scale` for NDFFT_NORM_SCALE), in one call.  The building block of spectral derivatives, de-aliasing
 * masks, filters, circular convolutions and Helmholtz solves along a periodic axis.
 *
 *   C2C plan   in, out: Complex<T>, lane length n, one `shape`, a stride vector each;   d_weights: n x Complex<T>
 *   R2C plan   in, out: REAL T, lane length n; meaning ndfft_r2c -> *= w -> ndifft_r2c, so Im(DC) and, for even n, Im(Nyquist) of the product are dropped as
 *              C2R always drops them;                                                   d_weights: (n / 2 + 1) x Complex<T>
 *   DCT plan   NDFFT_ERR_INVALID_ARG (the cosine pair has an entry point of its own: ndfft_exec_dct_filter_device below)
 *
 * Checks: those of ndfft_exec_device for the plan's forward op, with the same panic texts in the same order; then a NULL d_weights, then n_weights (the message
 * names both numbers), then unknown bits in `flags` (all NDFFT_ERR_INVALID_ARG).  A refused call launches nothing and writes nothing.
 * An array with a zero extent off the axis has no lane: as for ndfft_exec_device the call returns NDFFT_OK once the shapes agree, before it looks at the array
 * pointers, the weights or the flags, and writes nothing (the same holds for ndfft_exec_dct_filter_device).
 * d_in == d_out with identical strides is the in-place filter and is safe on every route; any other overlap is undefined, as for ndfft_exec_device.
 * Asynchronous on `stream`; d_weights is read on `stream`.
 *
 * Routes (ndfft_last_path):
 *   "filter_pow2"                      C2C plan, n = 64 .. 4096 a power of two, lanes on which ndfft_exec_device would run "pow2_reg" (unit stride along the axis in
 *                                      both arrays, lanes at a uniform pitch): ONE kernel, one read and one write of device memory per point, no scratch memory.
 *                                      Nothing is allocated except, at the first call of a plan whose radix list is no palindrome (f64 128, 1024, 2048; f32 2048), a
 *                                      second twiddle table: every other length can be captured into a HIP graph without a warm-up call.
 *   "filter_col_pow2"                  C2C plan, n = 128 .. 2048 a power of two, along a STRIDED axis: the fastest batch dimension has unit stride in both arrays
 *                                      (neighbouring lanes are adjacent: axis 0 of a 2-D C-layout array, the middle axis of a 3-D one, windows of either; the
 *                                      axis strides of the two arrays may differ), at least 8 lanes along it, at most two batch dimensions after merging: ONE
 *                                      kernel, a workgroup per tile of 4 .. 32 adjacent lanes staged through LDS, one read and one write of device memory per point,
 *                                      no scratch memory.  Allocates what "filter_pow2" allocates.
 *   "filter_r2c_pow2"                  R2C plan, n = 128 .. 8192 a power of two, unit stride along the axis in both arrays, lanes at a uniform pitch, both base
 *                                      pointers multiples of 2 * sizeof(T) and both lane pitches even (every lane starts on a whole complex element): ONE kernel
 *                                      on the real lane read as n / 2 complex points, one read and one write of device memory per real point, no scratch memory.
 *                                      The first filter call of a plan builds and uploads the kernel's twiddle tables; later calls allocate nothing, so one
 *                                      warm-up call is enough before a capture into a HIP graph.
 *   "<fwd route>+weights+<inv route>"  everything else, and every call with NDFFT_FILTER_NO_FUSE: forward transform into a dense spectrum image kept per host thread
 *                                      and stream, the diagonal pass in place on it, inverse transform into the output.  As for every multi-pass route the first call
 *                                      of a size allocates: warm a shape up before capturing it -- and capture it again once that (host thread, stream)'s scratch
 *                                      has been freed: by a later larger multi-pass call of the thread on the stream, ndfft_release_workspace or the thread's exit. */
#define NDFFT_FILTER_NO_FUSE 1   /* take the composed route even where a fused kernel exists (tests, A-B timing) */
int ndfft_exec_filter_device(const ndfft_plan *plan, const void *d_in, void *d_out, int ndim,
                             const int64_t *shape, const int64_t *stride_in, const int64_t *stride_out, int axis,
                             const void *d_weights, size_t n_weights, int norm, double scale, int flags, void *stream);

/* nddct_filter: for every lane along `axis`, out = s * DCT3(g (.) DCT2(in)) with the unnormalised lane definitions
 *   C[k] = sum_j x[j] cos(pi (2j+1) k / (2n)),     y[j] = D[0] / 2 + sum_{k >= 1} D[k] cos(pi (2j+1) k / (2n))
 * -- exactly what nddct2 -> lane *= g -> nddct3 give under the normalisation `norm`: s = 1 for NDFFT_NORM_NONE, 4 for NDFFT_NORM_DEFAULT (each of the two calls
 * pre-scales its input by 2), `scale` for NDFFT_NORM_SCALE.  Unit weights return s * (n / 2) * in.  The building block of cosine / Chebyshev-basis solvers on the Gauss
 * grid, Neumann-boundary Poisson and Helmholtz solves, de-aliasing and smoothing of non-periodic real data.
 *
 *   DCT plan   in, out: REAL T, lane length n, one `shape`, a stride vector each;   d_weights: n x T (REAL)
 *   C2C plan, R2C plan   NDFFT_ERR_INVALID_ARG
 *
 * The argument list, `flags`, in-place rule and asynchrony are those of ndfft_exec_filter_device.  Checks: those of ndfft_exec_device for NDFFT_OP_DCT2, with the same
 * panic texts in the same order ("Size mismatch in dct, got .. expected ..", the axis panic); then NULL array pointers, a NULL d_weights, n_weights != n (the message
 * names both numbers), unknown bits in `flags` (all NDFFT_ERR_INVALID_ARG).  A refused call launches nothing and writes nothing.
 *
 * Routes (ndfft_last_path):
 *   "filter_dct_pow2"                  n = 128 .. 8192 a power of two, unit stride along the axis in both arrays, lanes at a uniform pitch -- ANY base pointer and any
 *                                      pitch (16-byte accesses where both sides allow them, element-wide ones otherwise): ONE kernel, one read and one write of
 *                                      device memory per point, no scratch memory.  The first filter call of a plan builds and uploads the kernel's twiddle tables;
 *                                      later calls allocate nothing, so one warm-up call is enough before a capture into a HIP graph.
 *   "<dct2 route>+weights+<dct3 route>"  everything else, and every call with NDFFT_FILTER_NO_FUSE: DCT-II into a dense real image kept per host thread and stream, the
 *                                      diagonal pass in place on it, DCT-III into the output; the first call of a size allocates. */
int ndfft_exec_dct_filter_device(const ndfft_plan *plan, const void *d_in, void *d_out, int ndim,
                                 const int64_t *shape, const int64_t *stride_in, const int64_t *stride_out, int axis,
                                 const void *d_weights, size_t n_weights, int norm, double scale, int flags, void *stream);

#ifdef __cplusplus
}
#endif

/* ABI minor 7: ndfft_last_input_keep, ndfft_set_keep_budget, ndfft_force_input_keep -- declared in a header of their own */
#include "ndfft_mi355x_keep.h"

#endif /* NDFFT_MI355X_EXT_H */
